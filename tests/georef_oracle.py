"""Spherical azimuthal-equidistant (AEQD) maps restated for the tests of ``radar_processor_amd/georef.py`` and
``csrc/rg_georef.hip`` -- written from the formulas of ``include/radargrid_hip.h`` (``rg_georef``), never from either.

Two restatements:

* NumPy float64 (:func:`inverse`, :func:`forward`, :func:`place`): what the kernels are compared with;
* mpmath at 40 digits (:func:`mp_inverse`, :func:`mp_forward`, :func:`mp_place`): what the NumPy restatement and the host
  maps are compared with.  It takes the angular distance from ``acos``, which costs nothing at 40 digits.

and the scenes: a radar position, a grid origin, gates as float32 x / y in the radar's plane.  The gates are azimuths x the
ranges :data:`RANGES` plus :data:`N_NONFINITE` gates with a NaN or an infinity, shuffled by a fixed seed so that every
prefix holds a mix.  ``east_200km`` has 360 azimuths and 4 099 gates; the other scenes have 180 azimuths (2 183 gates), which
keeps the 40-digit evaluation of EVERY finite gate of EVERY scene within 20 000 evaluations (4 083 + 7 x 2 167 = 19 252).

    python tests/georef_oracle.py [--out PATH]        # the numbers of profiles/georef_bounds.json (kernel part: needs a GPU)
"""
from __future__ import annotations

import functools
import math
from typing import Dict, NamedTuple, Tuple

import numpy as np

R_EARTH = 6370997.0
RANGES = (0.0, 1.0, 120.0, 1.0e3, 1.0e4, 3.0e4, 6.0e4, 1.2e5, 2.4e5, 3.6e5, 4.8e5)
N_NONFINITE = 16
LENGTHS = (1, 255, 257, 4099)
RMA1 = (-64.19, -31.44)                 # lon, lat of the reference's RMA1 site


# ---- NumPy float64 -----------------------------------------------------------------------------------------------------------
def inverse(x, y, lon_c, lat_c, R=R_EARTH):
    """Plane (x, y) about (lon_c, lat_c) degrees -> (lon, lat) RADIANS, float64."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    lam_c, phi_c = np.radians(lon_c), np.radians(lat_c)
    rho = np.hypot(x, y)
    c = rho / R
    with np.errstate(invalid="ignore", divide="ignore"):
        lat = np.arcsin(np.clip(np.cos(c) * np.sin(phi_c) + y * np.sin(c) * np.cos(phi_c) / rho, -1.0, 1.0))
        lon = lam_c + np.arctan2(x * np.sin(c), rho * np.cos(phi_c) * np.cos(c) - y * np.sin(phi_c) * np.sin(c))
    return np.where(rho == 0, lam_c, lon), np.where(rho == 0, phi_c, lat)


def forward(lam, phi, lon_0, lat_0, R=R_EARTH):
    """(lam, phi) RADIANS -> plane (x, y) about (lon_0, lat_0) degrees, float64."""
    lam_0, phi_0 = np.radians(lon_0), np.radians(lat_0)
    d = lam - lam_0
    a = np.cos(phi) * np.sin(d)
    b = np.cos(phi_0) * np.sin(phi) - np.sin(phi_0) * np.cos(phi) * np.cos(d)
    q = np.sin(phi_0) * np.sin(phi) + np.cos(phi_0) * np.cos(phi) * np.cos(d)
    s = np.hypot(a, b)
    c = np.arctan2(s, q)
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(s == 0, 1.0, c / s)
    return R * k * a, R * k * b


def place(x32, y32, radar_lonlat, origin_lonlat, R=R_EARTH):
    """The contract of ``rg_gates_to_frame_f32`` in float64, BEFORE the one rounding to float32: the gates of a radar at
    ``radar_lonlat``, in the plane about ``origin_lonlat``, relative to the antenna's position there.  Returns
    ``(x', y', (ox, oy))``; NaN in both where x or y is not finite; the inputs themselves where the two positions are equal."""
    x32, y32 = np.asarray(x32, dtype=np.float32), np.asarray(y32, dtype=np.float32)
    if tuple(radar_lonlat) == tuple(origin_lonlat):
        return x32.astype(np.float64), y32.astype(np.float64), (0.0, 0.0)
    ox, oy = forward(*(np.radians(v) for v in radar_lonlat), *origin_lonlat, R)
    bad = ~(np.isfinite(x32) & np.isfinite(y32))
    lam, phi = inverse(np.where(bad, 0, x32), np.where(bad, 0, y32), *radar_lonlat, R)
    X, Y = forward(lam, phi, *origin_lonlat, R)
    return np.where(bad, np.nan, X - ox), np.where(bad, np.nan, Y - oy), (float(ox), float(oy))


def ulp_f32(v):
    """Spacing of float32 at ``float32(v)`` (elementwise, float64)."""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64).astype(np.float32))).astype(np.float64)


# ---- mpmath, 40 digits -------------------------------------------------------------------------------------------------------
def _mp():
    import mpmath
    mpmath.mp.dps = 40
    return mpmath


def mp_inverse(x, y, lon_c, lat_c, R=R_EARTH):
    """One point; exact conversions of the float64 arguments; (lam, phi) radians as mpf."""
    mp = _mp()
    x, y, R = mp.mpf(float(x)), mp.mpf(float(y)), mp.mpf(float(R))
    lam_c, phi_c = mp.radians(mp.mpf(float(lon_c))), mp.radians(mp.mpf(float(lat_c)))
    rho = mp.hypot(x, y)
    if rho == 0:
        return lam_c, phi_c
    c = rho / R
    phi = mp.asin(mp.cos(c) * mp.sin(phi_c) + y * mp.sin(c) * mp.cos(phi_c) / rho)
    lam = lam_c + mp.atan2(x * mp.sin(c), rho * mp.cos(phi_c) * mp.cos(c) - y * mp.sin(phi_c) * mp.sin(c))
    return lam, phi


def mp_forward(lam, phi, lon_0, lat_0, R=R_EARTH):
    """One point, (lam, phi) radians (mpf or float) -> (x, y) mpf."""
    mp = _mp()
    lam, phi, R = mp.mpf(lam), mp.mpf(phi), mp.mpf(float(R))
    lam_0, phi_0 = mp.radians(mp.mpf(float(lon_0))), mp.radians(mp.mpf(float(lat_0)))
    d = lam - lam_0
    a = mp.cos(phi) * mp.sin(d)
    b = mp.cos(phi_0) * mp.sin(phi) - mp.sin(phi_0) * mp.cos(phi) * mp.cos(d)
    q = mp.sin(phi_0) * mp.sin(phi) + mp.cos(phi_0) * mp.cos(phi) * mp.cos(d)
    s = mp.hypot(a, b)
    if s == 0:
        return R * a, R * b
    k = mp.acos(q) / s
    return R * k * a, R * k * b


def mp_place(x32, y32, radar_lonlat, origin_lonlat, R=R_EARTH) -> Tuple[np.ndarray, np.ndarray]:
    """:func:`place` of finite gates at 40 digits, rounded to float64 at the very end (the difference X - ox included)."""
    ox, oy = mp_forward(*(_mp().radians(_mp().mpf(float(v))) for v in radar_lonlat), *origin_lonlat, R)
    out = np.empty((2, len(x32)), dtype=np.float64)
    for i, (x, y) in enumerate(zip(x32, y32)):
        X, Y = mp_forward(*mp_inverse(x, y, *radar_lonlat, R), *origin_lonlat, R)
        out[0, i], out[1, i] = float(X - ox), float(Y - oy)
    return out[0], out[1]


# ---- scenes ------------------------------------------------------------------------------------------------------------------
class Scene(NamedTuple):
    name: str
    radar: Tuple[float, float]          # lon, lat (degrees)
    origin: Tuple[float, float]
    x: np.ndarray                       # float32 [n], the radar's plane
    y: np.ndarray

    @property
    def finite(self) -> np.ndarray:
        return np.isfinite(self.x) & np.isfinite(self.y)


def _offset(origin, east_m, north_m):
    """The point (east_m, north_m) of the plane about ``origin``, as (lon, lat) degrees -- by the maps above."""
    lam, phi = inverse(east_m, north_m, *origin)
    return float(np.degrees(lam)), float(np.degrees(phi))


# name -> (radar lon/lat, origin lon/lat, azimuths)
PLACEMENTS: Dict[str, tuple] = {
    "at_origin": (RMA1, RMA1, 180),
    "east_1m": (_offset(RMA1, 1.0, 0.0), RMA1, 180),
    "east_200km": (_offset(RMA1, 2.0e5, 0.0), RMA1, 360),
    "north_east_1000km": (_offset(RMA1, 1.0e6 / math.sqrt(2.0), 1.0e6 / math.sqrt(2.0)), RMA1, 180),
    "antimeridian": ((-179.9, 12.0), (179.9, 12.5), 180),
    "lat_80": ((22.0, 80.0), (15.0, 79.0), 180),
    "equator": ((10.3, 0.0), (9.0, -0.7), 180),
    "north_mid": ((7.5, 47.3), (8.9, 46.2), 180),
}
SCENES = tuple(PLACEMENTS)


@functools.lru_cache(maxsize=None)
def scene(name: str) -> Scene:
    radar, origin, n_az = PLACEMENTS[name]
    rng = np.random.default_rng(20260 + SCENES.index(name))
    az = np.radians(np.arange(n_az) * (360.0 / n_az) + 0.25)
    r = np.asarray(RANGES)[:, None]
    x = (r * np.sin(az)[None, :]).ravel()
    y = (r * np.cos(az)[None, :]).ravel()
    n_extra = (LENGTHS[-1] if n_az == 360 else 2183) - x.size - N_NONFINITE          # a few gates off the lattice of azimuths
    x = np.concatenate([x, rng.uniform(-4.8e5, 4.8e5, n_extra)]).astype(np.float32)
    y = np.concatenate([y, rng.uniform(-4.8e5, 4.8e5, n_extra)]).astype(np.float32)
    bad = np.array([np.nan, np.inf, -np.inf, np.nan], dtype=np.float32)
    bx = np.where(np.arange(N_NONFINITE) % 3 != 1, np.resize(bad, N_NONFINITE), np.float32(1234.5))
    by = np.where(np.arange(N_NONFINITE) % 3 != 0, np.resize(bad[::-1], N_NONFINITE), np.float32(-77.25))
    x, y = np.concatenate([x, bx]).astype(np.float32), np.concatenate([y, by]).astype(np.float32)
    order = rng.permutation(x.size)
    s = Scene(name, tuple(radar), tuple(origin), x[order], y[order])
    assert int((~s.finite).sum()) == N_NONFINITE
    return s


@functools.lru_cache(maxsize=None)
def placed(name: str):
    """(x', y') float64 of the scene by the NumPy restatement -- computed once, shared, never modified."""
    s = scene(name)
    x, y, _ = place(s.x, s.y, s.radar, s.origin)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def oracle_error(name: str) -> float:
    """Largest |NumPy restatement - mpmath| over the finite gates of a scene, metres (both coordinates)."""
    s = scene(name)
    x, y = placed(name)
    mx, my = mp_place(s.x[s.finite], s.y[s.finite], s.radar, s.origin)     # same centre: forward(inverse()) is the identity
    return float(max(np.abs(x[s.finite] - mx).max(), np.abs(y[s.finite] - my).max()))


def oracle_summary() -> dict:
    """The reference-side numbers of profiles/georef_bounds.json."""
    per_scene = {name: oracle_error(name) for name in SCENES}
    return {"per_scene_m": per_scene, "max_m": max(per_scene.values()),
            "finite_gates": int(sum(scene(n).finite.sum() for n in SCENES))}


# ---- the kernel against the restatement (GPU) --------------------------------------------------------------------------------
KERNEL_FLOOR_M = 1e-6      # |got - float32(want)| <= ulp_f32(want) + this


def kernel_differences(name: str, dev) -> dict:
    """``place_gates_device`` on a scene against :func:`placed`: per output value ``|got - float32(want)|`` and its
    allowance ``ulp_f32(want) + KERNEL_FLOOR_M``.  Returns the figures the test asserts and the profile records."""
    import radar_processor_amd as rg
    s = scene(name)
    want = placed(name)
    got = [t.cpu().numpy() for t in rg.place_gates_device(s.x, s.y, s.radar, s.origin, device=dev)]
    fin = s.finite
    diff = np.stack([np.abs(g[fin].astype(np.float64) - w[fin].astype(np.float32).astype(np.float64)) for g, w in zip(got, want)])
    allow = np.stack([ulp_f32(w[fin]) + KERNEL_FLOOR_M for w in want])
    if s.radar == s.origin:         # the copy: a gate that is not finite keeps its bits
        nonfinite_ok = all(g[~fin].tobytes() == src[~fin].tobytes() for g, src in zip(got, (s.x, s.y)))
    else:                           # NaN in both outputs
        nonfinite_ok = all(np.isnan(g[~fin]).all() for g in got)
    return {"max_diff_m": float(diff.max()), "values_differing": int((diff > 0).sum()), "values": int(diff.size),
            "worst_excess_m": float((diff - allow).max()), "nonfinite_as_contract": bool(nonfinite_ok)}


if __name__ == "__main__":
    import argparse
    import json
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rec = {"oracle_vs_mpmath": oracle_summary()}
    import torch
    if torch.cuda.is_available():
        rec["kernel_vs_oracle"] = {n: kernel_differences(n, torch.device("cuda", 0)) for n in SCENES}
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
