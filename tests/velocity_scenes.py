"""Velocity scenes, each built to reach one thing (tests/test_velocity_scenes.py checks them on the CPU, tests/test_gpu_velocity.py
runs the device over the same arrays).  The references (``velocity_oracle.dealias``) are computed once per process and shared."""
import functools
from typing import NamedTuple, Optional

import numpy as np

import velocity_oracle as vo


class Scene(NamedTuple):
    vel: np.ndarray                       # float32 [S][R][G] or [R][G]
    nyquist: object                       # a number, or one per sweep
    n_bands: int
    wrap: bool
    mask: Optional[np.ndarray] = None
    truth_folds: Optional[np.ndarray] = None          # int64: the fold that restores the truth, where the scene has one


def fold_into(truth, vn):
    """The truth folded into [-vn, vn) and the number of intervals that restores it."""
    k = np.floor((truth + vn) / (2.0 * vn))
    return (truth - k * 2.0 * vn).astype(np.float32), k.astype(np.int64)


def wind(R, G, vn, B, speed, wrap=True, holes=0.0, seed=0):
    """A uniform wind seen from the radar, rising with range: truth = speed * cos(az - 0.7) * linspace(0.6, 1, G)."""
    az = 2.0 * np.pi * np.arange(R) / R
    truth = speed * np.cos(az - 0.7)[:, None] * np.linspace(0.6, 1.0, G)[None, :]
    vel, k = fold_into(truth, vn)
    if holes:
        vel[np.random.default_rng(seed).random((R, G)) < holes] = np.nan
    return Scene(vel, vn, B, wrap, None, k)


#: the scenes on which the restatement recovers the true fold at EVERY valid gate (the CPU test shows it)
RECOVERING = ("wind_24x40", "wind_24x40_nowrap", "wind_36x65", "wind_36x65_holes")


@functools.lru_cache(maxsize=None)
def scenes():
    out = {
        "wind_24x40": wind(24, 40, 10.0, 3, 22.0),
        "wind_24x40_nowrap": wind(24, 40, 10.0, 3, 22.0, wrap=False),
        "wind_36x65": wind(36, 65, 10.0, 3, 22.0),
        "wind_36x65_holes": wind(36, 65, 8.0, 3, 19.0, holes=0.10, seed=0),
        # equality with the oracle only: isolated sets and the centring keep these from the truth
        "holes_25": wind(36, 65, 8.0, 3, 19.0, holes=0.25, seed=1)._replace(truth_folds=None),
        "three_rays": wind(3, 64, 10.0, 3, 22.0)._replace(truth_folds=None),
        "bands_8": wind(20, 33, 12.0, 8, 30.0)._replace(truth_folds=None),
        "bands_2": wind(20, 33, 12.0, 2, 30.0)._replace(truth_folds=None),
    }
    # two sweeps of different Nyquist velocity and a mask: a wavefront straddles the sweeps, nothing pairs across them
    a, b = wind(3, 65, 10.0, 3, 22.0), wind(3, 65, 6.5, 3, 15.0)
    mask = np.zeros((2, 3, 65), np.uint8)
    mask[0, 1, 10:14] = 1
    mask[1, :, 40] = 7
    out["two_sweeps"] = Scene(np.stack([a.vel, b.vel]), (10.0, 6.5), 3, True, mask)
    for R, G in ((1, 1), (1, 70), (70, 1), (5, 63), (5, 64), (5, 65)):
        out[f"wind_{R}x{G}"] = wind(R, G, 10.0, 3, 22.0)._replace(truth_folds=None)
    for R in (2, 3):
        for wrap in (False, True):
            s = wind(R, 64, 10.0, 3, 22.0, wrap=wrap)._replace(truth_folds=None)
            s.vel[0, :] = np.float32(-7.0)                       # row 0 and the last row in different bands along all 64 gates
            s.vel[R - 1, :] = np.float32(8.0)
            out[f"rows_{R}x64_{'wrap' if wrap else 'nowrap'}"] = s
    out["band_limits"] = band_limits()
    return out


def band_limits(vn=10.0, B=3):
    """v at -Vn, +Vn, +-0, every inner band edge and its float32 neighbours, just beyond +-Vn; NaN, +-inf, |v| > 16384 and masked
    gates, which make no edge and split regions.  One ray of values, repeated on three rays with the invalid gates staggered."""
    edge = [np.float32(-vn + 2.0 * vn * b / B) for b in range(B + 1)]
    vals = []
    for e in edge:
        vals += [np.nextafter(e, np.float32(-np.inf)), e, np.nextafter(e, np.float32(np.inf))]
    vals += [np.float32(0.0), np.float32(-0.0), np.float32(16384.0), np.float32(-16384.0), np.nextafter(np.float32(16384.0), np.float32(np.inf)),
             np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(1e30), np.float32(2.0 ** -17), np.float32(3.0 * 2.0 ** -17),
             np.float32(9.99), np.float32(-9.99), np.float32(25.0), np.float32(-31.0)]
    row = np.array(vals, np.float32)
    vel = np.stack([row, np.roll(row, 1), np.roll(row, 5), row[::-1].copy()])
    mask = np.zeros(vel.shape, np.uint8)
    mask[1, 3] = 1
    mask[2, ::7] = 255
    return Scene(vel, vn, B, True, mask)


def two_regions(axis, G=200, R=18, big=16000.0):
    """Two regions split along one boundary, with values near +-16384 on either side so that the border sums pass 2^32:
    ``axis == 'ray'``: rays 0 .. R/2 - 1 against the rest (with R = 18 and G = 200 the border's upper ray begins a wavefront: runs
    of 64, 64, 64, 8 lanes; the wrap seam gives 200 pairs again, in runs of 56, 64, 64, 16); ``axis == 'gate'``: gates below G / 2
    against the rest (no runs).  Returned as (values, regions) for the edge kernel."""
    values = np.empty((R, G), np.float32)
    region = np.empty((R, G), np.int32)
    ramp = (np.arange(R * G, dtype=np.float64).reshape(R, G) % 97) * 2.0 ** -7
    first = np.arange(R)[:, None] < R // 2 if axis == "ray" else np.arange(G)[None, :] < G // 2
    first = np.broadcast_to(first, (R, G))
    values[...] = np.where(first, big + ramp, -big - ramp)
    region[...] = np.where(first, 1, 2)
    return values, region


def checkerboard(R=16, G=24, vn=10.0):
    """Two bands in a checkerboard: every gate is its own region and every neighbour pair an edge."""
    y, x = np.mgrid[:R, :G]
    vel = np.where((y + x) % 2 == 0, -0.5 * vn, 0.5 * vn).astype(np.float32)
    vel += (np.arange(R * G, dtype=np.float32).reshape(R, G) % 13) * np.float32(0.125)
    return Scene(vel, vn, 2, True)


@functools.lru_cache(maxsize=None)
def reference(name):
    s = scenes()[name]
    return vo.dealias(s.vel, s.nyquist, s.n_bands, s.mask, s.wrap)
