"""The Web Mercator warp and the overview pyramid restated for the tests of ``radar_processor_amd/warp.py`` and
``csrc/rg_warp.hip`` -- written from the formulas of ``include/radargrid_hip.h`` (``rg_mercator_raster``), never from either.

* NumPy float64: :func:`pixel_map` (the plane position of every pixel of a raster), the two sampling rules
  (:func:`sample_nearest`, :func:`sample_bilinear`) and the two overview rules (:func:`overview_nearest`,
  :func:`overview_average`): what the kernels are compared with;
* mpmath at 40 digits: :func:`mp_pixel` -- what :func:`pixel_map` is compared with (tests/test_warp_oracle.py);
* the scenes, their sources, and the pixels whose outcome rounding may decide either way (:func:`undecided_nearest`,
  :func:`undecided_bilinear`): at most :data:`UNDECIDED_CAP` of a scene's pixels, asserted on the CPU for every scene.

Source values are ``iy * 1000 + ix`` as float32, and for RGBA the same two indices packed into the bytes: a nearest sample
names its source pixel exactly, so a north / south or row / column flip cannot pass.
"""
from __future__ import annotations

import functools
import math
from typing import Dict, NamedTuple, Tuple

import numpy as np

A_MERCATOR = 6378137.0
R_EARTH = 6370997.0
LIMIT = math.pi / 2.0 - 0.1            # angular distance from the origin at and beyond which a pixel is fill
EDGE_EPS = 1e-6                        # fx + 0.5, fy + 0.5 this close to an integer, or wsum this close to 0.5: undecided
ANGLE_EPS = 1e-9                       # c this close to LIMIT: undecided
UNDECIDED_CAP = 1e-3                   # of a scene's pixels
PLANE_FLOOR_M = 1e-6                   # the plane-coordinate floor derived in tests/test_gpu_georef.py
FACTORS = (2, 4, 8, 16, 64)


class Raster(NamedTuple):              # field for field the rg_mercator_raster
    x_min: float
    y_max: float
    pixel: float
    width: int
    height: int


class Lattice(NamedTuple):             # field for field the rg_warp_source
    x_lo: float
    y_lo: float
    step_x: float
    step_y: float
    ny: int
    nx: int


def lattice(shape, limits) -> Lattice:
    (ny, nx), ((y0, y1), (x0, x1)) = shape, limits
    return Lattice(float(x0), float(y0), (x1 - x0) / (nx - 1), (y1 - y0) / (ny - 1), ny, nx)


# ---- NumPy float64 -----------------------------------------------------------------------------------------------------------
def pixel_map(raster: Raster, origin, R=R_EARTH):
    """``(Xg, Yg, c)`` float64 ``[height, width]``: every pixel centre in the AEQD plane about ``origin`` (lon, lat
    degrees), metres, and its angular distance from the origin."""
    lam0, phi0 = np.radians(origin[0]), np.radians(origin[1])
    X = raster.x_min + (np.arange(raster.width, dtype=np.float64) + 0.5) * raster.pixel
    Y = raster.y_max - (np.arange(raster.height, dtype=np.float64) + 0.5) * raster.pixel
    t = (Y / A_MERCATOR)[:, None]
    sp, cp = np.tanh(t), 1.0 / np.cosh(t)
    d = (X / A_MERCATOR - lam0)[None, :]
    sd, cd = np.sin(d), np.cos(d)
    a = cp * sd
    b = np.cos(phi0) * sp - np.sin(phi0) * cp * cd
    q = np.sin(phi0) * sp + np.cos(phi0) * cp * cd
    s = np.hypot(a, b)
    c = np.arctan2(s, q)
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(s == 0, 1.0, c / s)
    return R * k * a, R * k * b, c


def node_coords(Xg, Yg, lat: Lattice):
    return (Xg - lat.x_lo) / lat.step_x, (Yg - lat.y_lo) / lat.step_y


def nearest_index(fx, fy, c, lat: Lattice):
    """``(inside, iy, ix)`` of the nearest rule."""
    ix, iy = np.floor(fx + 0.5), np.floor(fy + 0.5)
    inside = (c < LIMIT) & (ix >= 0) & (ix < lat.nx) & (iy >= 0) & (iy < lat.ny)
    return inside, np.where(inside, iy, 0).astype(np.int64), np.where(inside, ix, 0).astype(np.int64)


def sample_nearest(src, fx, fy, c, lat: Lattice, fill):
    """``src`` float32 ``[P, ny, nx]`` -> ``[P, H, W]`` (bits copied; ``fill`` outside), or uint8 ``[ny, nx, 4]`` ->
    ``[H, W, 4]`` (zeros outside)."""
    inside, iy, ix = nearest_index(fx, fy, c, lat)
    if src.dtype == np.uint8:
        return np.where(inside[..., None], src[iy, ix], np.uint8(0))
    bits = src.view(np.uint32)[:, iy, ix]
    return np.where(inside[None], bits, np.float32(fill).reshape(1).view(np.uint32)[0]).view(np.float32)


def sample_bilinear(plane, fx, fy, c, lat: Lattice, fill):
    """One float32 plane ``[ny, nx]`` -> ``(out float64 [H, W] BEFORE the rounding to float32, wsum, filled)``; ``filled``
    marks the pixels that are ``fill`` (their ``out`` is NaN)."""
    x0, y0 = np.floor(fx), np.floor(fy)
    tx, ty = fx - x0, fy - y0
    weights = ((1 - ty) * (1 - tx), (1 - ty) * tx, ty * (1 - tx), ty * tx)
    wsum, vsum = np.zeros_like(fx), np.zeros_like(fx)
    for (dy, dx), w in zip(((0, 0), (0, 1), (1, 0), (1, 1)), weights):
        yy, xx = y0 + dy, x0 + dx
        ok = (yy >= 0) & (yy < lat.ny) & (xx >= 0) & (xx < lat.nx)
        v = plane[np.where(ok, yy, 0).astype(np.int64), np.where(ok, xx, 0).astype(np.int64)].astype(np.float64)
        ok &= ~np.isnan(v)
        wsum = wsum + np.where(ok, w, 0.0)
        vsum = vsum + np.where(ok, w * np.where(ok, v, 0.0), 0.0)
    wsum = np.where(c < LIMIT, wsum, 0.0)
    filled = ~(wsum >= 0.5)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(filled, np.nan, vsum / wsum), wsum, filled


def overview_shape(h, w, f):
    return -(-h // f), -(-w // f)


def overview_nearest(img, f):
    """``img`` ``[.., h, w]`` (float32 planes) or ``[h, w, 4]`` uint8."""
    rgba = img.dtype == np.uint8
    h, w = img.shape[:2] if rgba else img.shape[-2:]
    oh, ow = overview_shape(h, w, f)
    rows = np.minimum(np.arange(oh) * f + f // 2, h - 1)
    cols = np.minimum(np.arange(ow) * f + f // 2, w - 1)
    return img[rows[:, None], cols[None, :]] if rgba else img[..., rows[:, None], cols[None, :]]


def overview_average(img, f):
    """float32 ``[.., h, w]`` -> float64 means BEFORE the rounding to float32 (NaN: no finite value in the block); the sum
    runs in float64 over the block in row-major order, one value after the other."""
    planes = img.reshape((-1,) + img.shape[-2:])
    h, w = planes.shape[-2:]
    oh, ow = overview_shape(h, w, f)
    out = np.full((planes.shape[0], oh, ow), np.nan)
    for p in range(planes.shape[0]):
        for r in range(oh):
            for c in range(ow):
                total, count = 0.0, 0
                for v in planes[p, r * f:min((r + 1) * f, h), c * f:min((c + 1) * f, w)].ravel().tolist():
                    if math.isfinite(v):
                        total += v
                        count += 1
                if count:
                    out[p, r, c] = total / count
    return out.reshape(img.shape[:-2] + (oh, ow))


def ulp_f32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64).astype(np.float32))).astype(np.float64)


# ---- mpmath, 40 digits -------------------------------------------------------------------------------------------------------
def _mp():
    import mpmath
    mpmath.mp.dps = 40
    return mpmath


def mp_pixel(raster: Raster, origin, r: int, c: int, R=R_EARTH):
    """``(Xg, Yg)`` of pixel (r, c) as mpf; the float64 members are converted exactly, the angular distance is ``acos``."""
    mp = _mp()
    X = mp.mpf(raster.x_min) + (mp.mpf(c) + mp.mpf("0.5")) * mp.mpf(raster.pixel)
    Y = mp.mpf(raster.y_max) - (mp.mpf(r) + mp.mpf("0.5")) * mp.mpf(raster.pixel)
    t = Y / mp.mpf(A_MERCATOR)
    sp, cp = mp.tanh(t), 1 / mp.cosh(t)
    lam0, phi0 = mp.radians(mp.mpf(float(origin[0]))), mp.radians(mp.mpf(float(origin[1])))
    d = X / mp.mpf(A_MERCATOR) - lam0
    a = cp * mp.sin(d)
    b = mp.cos(phi0) * sp - mp.sin(phi0) * cp * mp.cos(d)
    q = mp.sin(phi0) * sp + mp.cos(phi0) * cp * mp.cos(d)
    s = mp.hypot(a, b)
    k = mp.acos(q) / s if s != 0 else mp.mpf(1)
    return mp.mpf(float(R)) * k * a, mp.mpf(float(R)) * k * b


# ---- scenes ------------------------------------------------------------------------------------------------------------------
class Scene(NamedTuple):
    name: str
    shape: Tuple[int, int]                       # ny, nx of the source
    limits: tuple                                # ((y0, y1), (x0, x1)), metres
    origin: Tuple[float, float]                  # lon, lat
    raster: Raster

    @property
    def lattice(self) -> Lattice:
        return lattice(self.shape, self.limits)

    @property
    def pixels(self) -> int:
        return self.raster.width * self.raster.height


RMA1 = (-64.19, -31.44)
WIDE = ((-168e3, 168e3), (-240e3, 240e3))
# name -> (shape, limits, origin); the raster of these is mercator_raster_for's
GRIDS: Dict[str, tuple] = {
    "rma1": ((37, 53), WIDE, RMA1),
    "lat_70": ((37, 53), WIDE, (10.0, 70.0)),
    "antimeridian": ((33, 41), ((-84e3, 84e3), (-120e3, 120e3)), (-179.5, 5.0)),
}
MAIN = tuple(GRIDS)                              # the scenes evaluated at 40 digits, and the overview inputs
SCENES = MAIN + ("rma1_fine", "one_pixel", "one_row", "one_column", "tile_edge", "far_hemisphere")


def tile_raster(z, x, y, size) -> Raster:
    """XYZ tile, restated: edges at ``2 pi a (i / 2^z - 1/2)``."""
    world, n = 2.0 * math.pi * A_MERCATOR, 1 << z
    return Raster(world * (x / n - 0.5), world * (0.5 - y / n), world / n / size, size, size)


@functools.lru_cache(maxsize=None)
def scene(name: str) -> Scene:
    import radar_processor_amd as rg
    if name in GRIDS:
        shape, limits, origin = GRIDS[name]
        return Scene(name, shape, limits, origin, Raster(*rg.mercator_raster_for(shape, limits, origin)))
    base = scene("rma1")
    r = base.raster
    if name == "rma1_fine":                      # several tiles of the kernel in both directions
        return base._replace(name=name, raster=Raster(*rg.mercator_raster_for(base.shape, base.limits, base.origin,
                                                                               pixel_size=r.pixel / 3.0)))
    if name == "one_pixel":
        return base._replace(name=name, raster=Raster(r.x_min + 10.3 * r.pixel, r.y_max - 7.7 * r.pixel, r.pixel, 1, 1))
    if name == "one_row":
        return base._replace(name=name, raster=Raster(r.x_min, r.y_max - 11.4 * r.pixel, r.pixel, r.width, 1))
    if name == "one_column":
        return base._replace(name=name, raster=Raster(r.x_min + 20.6 * r.pixel, r.y_max, r.pixel, 1, r.height))
    if name == "tile_edge":                      # the zoom-6 tile that holds the grid's south-west corner node, 64 x 64
        x, y = r.x_min + 0.5 * r.pixel, r.y_max - (r.height - 0.5) * r.pixel
        world = 2.0 * math.pi * A_MERCATOR
        return base._replace(name=name, raster=tile_raster(6, int((x / world + 0.5) * 64), int((0.5 - y / world) * 64), 64))
    if name == "far_hemisphere":                 # the contract scene: the plane holds the whole sphere, the limit must cut it
        return Scene(name, (9, 9), ((-2e7, 2e7), (-2e7, 2e7)), (10.0, 20.0), tile_raster(0, 0, 0, 256))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def mapped(name: str):
    """``(fx, fy, c)`` of a scene by the NumPy restatement -- computed once, shared, never modified."""
    s = scene(name)
    Xg, Yg, c = pixel_map(s.raster, s.origin)
    fx, fy = node_coords(Xg, Yg, s.lattice)
    for a in (fx, fy, c):
        a.setflags(write=False)
    return fx, fy, c


def index_plane(shape) -> np.ndarray:
    ny, nx = shape
    return (np.arange(ny, dtype=np.float32)[:, None] * np.float32(1000.0) + np.arange(nx, dtype=np.float32)[None, :])


def index_rgba(shape) -> np.ndarray:
    """``[ny, nx, 4]`` uint8: iy, ix, their high bits (none at these sizes), and 255 -- a source pixel is never 0, 0, 0, 0."""
    ny, nx = shape
    iy, ix = np.broadcast_arrays(np.arange(ny)[:, None], np.arange(nx)[None, :])
    return np.ascontiguousarray(np.stack([iy & 255, ix & 255, (iy >> 8) | ((ix >> 8) << 4), np.full_like(iy, 255)],
                                         axis=-1).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def planes(name: str, n_planes: int) -> np.ndarray:
    """float32 ``[n_planes, ny, nx]``: plane 0 is ``iy * 1000 + ix``; plane 1 its negative with a NaN (payload kept) and
    both infinities planted; plane 2 is plane 0 plus a half."""
    base = index_plane(scene(name).shape)
    out = np.stack([base, -base, base + np.float32(0.5)][:n_planes]).astype(np.float32)
    if n_planes > 1:
        out[1, 3, 4], out[1, 5, 2] = np.inf, -np.inf
        out[1].view(np.uint32)[4, 6] = 0x7FC12345
    out.setflags(write=False)
    return out


BILINEAR_SOURCES = ("clean", "nan_30_percent", "nan_checkerboard", "one_finite")


@functools.lru_cache(maxsize=None)
def bilinear_source(name: str, kind: str) -> np.ndarray:
    s = scene(name)
    v = index_plane(s.shape).copy()
    ny, nx = s.shape
    if kind == "nan_30_percent":
        v[np.random.default_rng(3030 + SCENES.index(name)).random(s.shape) < 0.3] = np.nan
    elif kind == "nan_checkerboard":
        v[(np.arange(ny)[:, None] + np.arange(nx)[None, :]) % 2 == 1] = np.nan
    elif kind == "one_finite":
        keep = v[ny // 2, nx // 3]
        v[:] = np.nan
        v[ny // 2, nx // 3] = keep
    elif kind != "clean":
        raise KeyError(kind)
    v.setflags(write=False)
    return v


def adjacent_difference(plane) -> float:
    """D: the largest difference between two finite taps of one 2 x 2 cell."""
    cells = np.stack([plane[:-1, :-1], plane[:-1, 1:], plane[1:, :-1], plane[1:, 1:]]).astype(np.float64)
    any_finite = np.isfinite(cells).any(axis=0)
    hi = np.where(any_finite, np.nanmax(np.where(np.isfinite(cells), cells, -np.inf), axis=0), 0.0)
    lo = np.where(any_finite, np.nanmin(np.where(np.isfinite(cells), cells, np.inf), axis=0), 0.0)
    return float((hi - lo).max())


def bilinear_allowance(name: str, want, plane) -> np.ndarray:
    """``ulp_f32(want) + 2 * (1e-6 m / min(step)) * D``: the coordinate floor in pixels, once per axis."""
    lat = scene(name).lattice
    return ulp_f32(want) + 2.0 * (PLANE_FLOOR_M / min(lat.step_x, lat.step_y)) * adjacent_difference(plane)


def _near_integer(v, eps):
    return np.abs(v - np.round(v)) < eps


def undecided_nearest(name: str) -> np.ndarray:
    fx, fy, c = mapped(name)
    return _near_integer(fx + 0.5, EDGE_EPS) | _near_integer(fy + 0.5, EDGE_EPS) | (np.abs(c - LIMIT) < ANGLE_EPS)


def undecided_bilinear(name: str, plane) -> np.ndarray:
    fx, fy, c = mapped(name)
    _, wsum, _ = sample_bilinear(plane, fx, fy, np.zeros_like(c), scene(name).lattice, np.nan)     # wsum before the limit
    return (np.abs(wsum - 0.5) < EDGE_EPS) | (np.abs(c - LIMIT) < ANGLE_EPS)


def nearest_candidates(name: str, src, fill):
    """The outcomes an undecided pixel may take: the sample at ``(fx +- 2 EDGE_EPS, fy +- 2 EDGE_EPS)`` and, near the
    angular limit, the fill.  A list of arrays shaped like the result."""
    s = scene(name)
    fx, fy, c = mapped(name)
    out = []
    for dx in (-2 * EDGE_EPS, 2 * EDGE_EPS):
        for dy in (-2 * EDGE_EPS, 2 * EDGE_EPS):
            for cc in (c, c - 2 * ANGLE_EPS, c + 2 * ANGLE_EPS):
                out.append(sample_nearest(src, fx + dx, fy + dy, cc, s.lattice, fill))
    return out


# ---- overview inputs ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def overview_input(name: str) -> np.ndarray:
    """float32 ``[2, H, W]`` at the size of a main scene's raster: plane 0 smooth values with NaN outside a disc, an
    all-NaN 16 x 16 corner, a block with one finite value, and both infinities; plane 1 random with 30 % NaN."""
    r = scene(name).raster
    h, w = r.height, r.width
    rng = np.random.default_rng(77 + MAIN.index(name))
    yy, xx = np.mgrid[0:h, 0:w]
    a = (20.0 + 0.37 * yy - 0.21 * xx + rng.normal(0.0, 3.0, (h, w))).astype(np.float32)
    a[(yy - h / 2.0) ** 2 + (xx - w / 2.0) ** 2 > (0.45 * w) ** 2] = np.nan
    a[:16, :16] = np.nan                                  # all-NaN blocks at every factor up to 16
    a[16:32, 16:32] = np.nan
    a[21, 27] = np.float32(42.5)                          # ... and a block with a single finite value
    a[h // 2, w // 2], a[h // 2 + 1, w // 2 - 3] = np.inf, -np.inf
    b = rng.uniform(-30.0, 70.0, (h, w)).astype(np.float32)
    b[rng.random((h, w)) < 0.3] = np.nan
    out = np.stack([a, b])
    out.setflags(write=False)
    return out


# ---- the numbers of profiles/warp_bounds.json --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_error(name: str) -> float:
    """Largest |NumPy restatement - mpmath| over every pixel of a scene, metres in the plane (both coordinates)."""
    s = scene(name)
    Xg, Yg, _ = pixel_map(s.raster, s.origin)
    worst = 0.0
    for r in range(s.raster.height):
        for c in range(s.raster.width):
            mx, my = mp_pixel(s.raster, s.origin, r, c)
            worst = max(worst, abs(float(mx - _mp().mpf(float(Xg[r, c])))), abs(float(my - _mp().mpf(float(Yg[r, c])))))
    return worst


def oracle_summary() -> dict:
    per_scene = {name: oracle_error(name) for name in MAIN}
    return {"per_scene_m": per_scene, "max_m": max(per_scene.values()), "pixels": int(sum(scene(n).pixels for n in MAIN))}


def bilinear_differences(name: str, kind: str, dev) -> dict:
    """``warp_to_mercator_device(method="bilinear")`` on one source of a scene against :func:`sample_bilinear`: the fill
    set (undecided pixels aside) and, per kept pixel, ``|got - float32(want)|`` against :func:`bilinear_allowance`."""
    import radar_processor_amd as rg
    s = scene(name)
    plane = bilinear_source(name, kind)
    fx, fy, c = mapped(name)
    want, _, filled = sample_bilinear(plane, fx, fy, c, s.lattice, np.nan)
    got = rg.warp_to_mercator_device(plane, s.limits, s.origin, s.raster, method="bilinear", device=dev).cpu().numpy()
    decided = ~undecided_bilinear(name, plane)
    both = decided & ~filled & ~np.isnan(got)
    diff = np.abs(got[both].astype(np.float64) - want[both].astype(np.float32).astype(np.float64))
    allow = bilinear_allowance(name, want[both], plane)
    return {"pixels": int(filled.size), "kept": int((~filled).sum()), "undecided": int((~decided).sum()),
            "fill_set_differs": int((np.isnan(got) != filled)[decided].sum()),
            "max_diff": float(diff.max(initial=0.0)), "values_differing": int((diff > 0).sum()),
            "worst_excess": float((diff - allow).max(initial=-np.inf)) if diff.size else None}


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
        rec["bilinear_vs_oracle"] = {n: {k: bilinear_differences(n, k, torch.device("cuda", 0)) for k in BILINEAR_SOURCES}
                                     for n in SCENES}
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
