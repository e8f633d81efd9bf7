"""Rim cases for the ROI neighbour search -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The fused ROI kernel (``roi_block_kernel``, radar_processor_amd/csrc/rg_roi_grid.hip) decides membership with a float32
distance and falls back to the reference's float64 ``d2 < r2`` (src/radar_grid/compute.py:69-74) only inside a band of
about 2e-6 around the rim.  Random clouds land in that band about once per million pairs, so this module PLANTS gates
there: float32 gate coordinates are nudged by ulps around points at distance ``r`` of a voxel until the float64 and the
kernel's float32 distance fall where a case wants them, and every planted gate is labelled with the case it covers:

  A  float64 inside, float32 ``d2f >= r2f`` (the float32 Cressman weight would be <= 0)
  B  float64 inside, float32 in the band, ``d2f < r2f``
  C  float64 outside, float32 in the band, ``d2f < r2f`` (float32 alone would admit it)
  D  ``d2 == r2`` exactly (integer Pythagorean offsets at an integer radius): the strict ``<`` rejects it
  E  ``d2f`` within a few float32 ulps of ``r2_lo`` or ``r2_hi``, where float32 alone decides

Voxel coordinates come from :func:`radar_grid_oracle.axis_coords_f32`, ``r`` from the oracle's float64 formula
(compute.py:46-47).  The kernel's float32 quantities are emulated exactly: ``dx = fl32(g.x - xf)``, then
``fmaf(dz, dz, fmaf(dy, dy, dx * dx))`` with each fmaf rounded ONCE (:func:`d2f_kernel` rounds through float64 with
round-to-odd, :func:`d2f_exact` through ``fractions.Fraction``; the tests check that the two agree).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from fractions import Fraction
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from .radar_grid_oracle import axis_coords_f32

CASES = ("A", "B", "C", "D", "E")
E_ULPS = 4                     # case E: d2f within this many float32 ulps of r2_lo or r2_hi

_F32 = np.float32
_ONE_HI = _F32(1.0) + _F32(2.4e-7)     # (1.0f + 2.4e-7f), rg_roi_grid.hip
_ONE_LO = _F32(1.0) - _F32(2.4e-7)


# --------------------------------------------------------------------------------------------------
# the kernel's float32 arithmetic, emulated exactly
# --------------------------------------------------------------------------------------------------
def _round_f32_exact(q: Fraction) -> np.float32:
    """Round a rational to the nearest float32, ties to even (one rounding)."""
    c = _F32(float(q))                 # within one float32 ulp of the answer (float64 first can round twice)
    best = None
    for cand in (np.nextafter(c, _F32(-np.inf)), c, np.nextafter(c, _F32(np.inf))):
        err = abs(Fraction(float(cand)) - q)
        key = (err, int(np.array(cand, dtype=np.float32).view(np.uint32)) & 1)
        if best is None or key < best[0]:
            best = (key, cand)
    return _F32(best[1])


def d2f_exact(gx, gy, gz, xf, yf, zf) -> np.float32:
    """The kernel's float32 d2 for ONE (gate, voxel) pair, fmaf evaluated with exact rationals."""
    dx = _F32(gx) - _F32(xf)
    dy = _F32(gy) - _F32(yf)
    dz = _F32(gz) - _F32(zf)
    p = dx * dx
    s = _round_f32_exact(Fraction(float(dy)) ** 2 + Fraction(float(p)))
    return _round_f32_exact(Fraction(float(dz)) ** 2 + Fraction(float(s)))


def _fmaf(a: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    """Vectorised fmaf for float32 arrays: a*b is exact in float64; a*b + c is rounded to odd in float64 (TwoSum tells
    whether it was exact), which makes the final rounding to float32 a single correct one (53 >= 24 + 2)."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c64 = c.astype(np.float64)
    s = p + c64
    bp = s - c64
    err = (p - bp) + (c64 - (s - bp))                   # TwoSum: p + c = s + err exactly
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def d2f_kernel(gx, gy, gz, xf, yf, zf) -> np.ndarray:
    """The kernel's float32 d2 (rg_roi_grid.hip, dense stage), vectorised."""
    dx = np.asarray(gx, dtype=np.float32) - _F32(xf)
    dy = np.asarray(gy, dtype=np.float32) - _F32(yf)
    dz = np.asarray(gz, dtype=np.float32) - _F32(zf)
    return _fmaf(dz, dz, _fmaf(dy, dy, dx * dx))


@dataclass(frozen=True)
class Rim:
    """One voxel's float64 ROI and the kernel's float32 thresholds derived from it."""
    x: float
    y: float
    z: float
    r2: float
    r2f: np.float32
    r2_lo: np.float32
    r2_hi: np.float32


def voxel_rim(x: float, y: float, z: float, min_radius: float, beam_factor: float) -> Rim:
    """compute.py:46-47 in float64 from the float32 voxel centre; r2_lo / r2_hi as rg_roi_grid.hip computes them."""
    x, y, z = float(_F32(x)), float(_F32(y)), float(_F32(z))
    r = max(min_radius, float(np.sqrt(x * x + y * y + z * z)) * beam_factor)
    r2 = r * r
    return Rim(x, y, z, r2, _F32(r2), r2_lo=_F32(r2 * (1.0 - 2e-6)) * _ONE_LO, r2_hi=_F32(r2 * (1.0 + 2e-6)) * _ONE_HI)


def d2_f64(gx, gy, gz, x, y, z) -> np.ndarray:
    """The reference's float64 d2 (compute.py:69-72) from float32 gate coordinates."""
    ex = np.asarray(gx, dtype=np.float32).astype(np.float64) - x
    ey = np.asarray(gy, dtype=np.float32).astype(np.float64) - y
    ez = np.asarray(gz, dtype=np.float32).astype(np.float64) - z
    return ex * ex + ey * ey + ez * ez


def _ulp_distance(a: np.ndarray, b: np.float32) -> np.ndarray:
    """Signed distance in float32 ulps between positive float32 values."""
    return np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64) - int(np.array(b, np.float32).view(np.int32))


def classify(gx, gy, gz, rim: Rim) -> np.ndarray:
    """Case label ('A'..'E', '' for none) of every gate against one voxel; priority D > A > C > B > E."""
    d2 = d2_f64(gx, gy, gz, rim.x, rim.y, rim.z)
    d2f = d2f_kernel(gx, gy, gz, rim.x, rim.y, rim.z)
    inside = d2 < rim.r2
    band = (d2f > rim.r2_lo) & (d2f <= rim.r2_hi)
    near_edge = ((np.abs(_ulp_distance(d2f, rim.r2_lo)) <= E_ULPS) | (np.abs(_ulp_distance(d2f, rim.r2_hi)) <= E_ULPS))
    lab = np.full(d2.shape, "", dtype="<U1")
    lab[near_edge] = "E"
    lab[inside & band & (d2f < rim.r2f)] = "B"
    lab[~inside & band & (d2f < rim.r2f)] = "C"
    lab[inside & (d2f >= rim.r2f)] = "A"
    lab[d2 == rim.r2] = "D"
    return lab


# --------------------------------------------------------------------------------------------------
# planting
# --------------------------------------------------------------------------------------------------
def _ulp_steps(v: np.float32, k: int) -> np.ndarray:
    """v and its k float32 neighbours on each side."""
    out = [v]
    lo = hi = v
    for _ in range(k):
        lo = np.nextafter(lo, _F32(-np.inf)); hi = np.nextafter(hi, _F32(np.inf))
        out = [lo] + out + [hi]
    return np.array(out, dtype=np.float32)


def _lattice(p: np.ndarray, k: int, axes=(0, 1, 2)) -> np.ndarray:
    """All points within k ulps of float32 point p along the given axes, [N, 3] float32."""
    cols = [(_ulp_steps(_F32(p[a]), k) if a in axes else np.array([_F32(p[a])])) for a in range(3)]
    g = np.meshgrid(*cols, indexing="ij")
    return np.stack([c.ravel() for c in g], axis=1)


@functools.lru_cache(maxsize=8)
def pythagorean_offsets(r: int) -> np.ndarray:
    """Every integer (a, b, c) with a^2 + b^2 + c^2 == r^2 (all sign and axis variants), [N, 3] float64."""
    out = []
    for a in range(0, r + 1):
        for b in range(a, r + 1):
            c2 = r * r - a * a - b * b
            if c2 < b * b:
                break
            c = int(round(c2 ** 0.5))
            if c * c == c2:
                base = (a, b, c)
                for perm in {(base[i], base[j], base[k]) for i, j, k in
                             ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))}:
                    for sx in (1, -1):
                        for sy in (1, -1):
                            for sz in (1, -1):
                                out.append((sx * perm[0], sy * perm[1], sz * perm[2]))
    return np.unique(np.array(out, dtype=np.float64), axis=0)


def plant(rim: Rim, case: str, rng: np.random.Generator, direction: Optional[str] = None, tries: int = 40,
          k: int = 3) -> Optional[np.ndarray]:
    """One float32 gate (x, y, z) of the given case for this voxel, or None when ``tries`` directions found none.

    ``direction``: None = uniform on the sphere; 'out:<signs>' = only directions whose components have the given signs
    ('+', '-' or '.' for any; e.g. 'out:+-.'), used for gates beyond the grid's faces; 'up' / 'down' = straight above /
    below the voxel (only the z coordinate is nudged, so the case is whatever the z lattice reaches: pass case '<' for
    the innermost gate inside the rim or '>' for the outermost one outside it)."""
    c = np.array([rim.x, rim.y, rim.z])
    r = float(np.sqrt(rim.r2))
    if direction in ("up", "down"):
        s = 1.0 if direction == "up" else -1.0
        z0 = _F32(rim.z + s * r)
        zs = _ulp_steps(z0, 64)
        gx = np.full(zs.shape, _F32(rim.x)); gy = np.full(zs.shape, _F32(rim.y))
        d2 = d2_f64(gx, gy, zs, rim.x, rim.y, rim.z)
        inside = d2 < rim.r2
        if case == "<":
            pick = np.nonzero(inside)[0]
            j = pick[np.argmax(d2[pick])] if pick.size else None
        else:
            pick = np.nonzero(~inside)[0]
            j = pick[np.argmin(d2[pick])] if pick.size else None
        return None if j is None else np.array([gx[j], gy[j], zs[j]], dtype=np.float32)
    if case == "D":
        ri = int(round(np.sqrt(rim.r2)))
        if ri * ri != rim.r2 or any(v != round(v) for v in (rim.x, rim.y, rim.z)):
            return None
        offs = pythagorean_offsets(ri)
        if direction is not None:
            offs = offs[_sign_ok(offs, direction)]
        if offs.size == 0:
            return None
        o = offs[rng.integers(offs.shape[0])]
        return (c + o).astype(np.float32)
    if case == "E":
        target = float(rim.r2_lo if rng.random() < 0.5 else rim.r2_hi)
    else:
        target = rim.r2
    for _ in range(tries):
        u = rng.normal(size=3)
        if direction is not None:
            u = _signs(direction, u)
        u /= np.linalg.norm(u)
        p = (c + u * np.sqrt(target)).astype(np.float32)
        cand = _lattice(p, k)
        lab = classify(cand[:, 0], cand[:, 1], cand[:, 2], rim)
        hit = np.nonzero(lab == case)[0]
        if hit.size:
            return cand[hit[rng.integers(hit.size)]]
    return None


def _signs(direction: str, u: np.ndarray) -> np.ndarray:
    """u with the signs 'out:<xyz>' asks for ('+', '-', or '.' = keep u's own)."""
    spec = direction.split(":", 1)[1]
    return np.array([abs(v) if s == "+" else -abs(v) if s == "-" else v for v, s in zip(u, spec)])


def _sign_ok(offs: np.ndarray, direction: str) -> np.ndarray:
    spec = direction.split(":", 1)[1]
    ok = np.ones(offs.shape[0], dtype=bool)
    for a, s in enumerate(spec):
        if s == "+":
            ok &= offs[:, a] > 0
        elif s == "-":
            ok &= offs[:, a] < 0
    return ok


@dataclass
class RimCloud:
    """Planted gates: float32 coordinates (z relative to the radar, as the search sees it), the flat index of the voxel
    each one was planted for and its case label against that voxel ('' = none of A-E)."""
    gx: np.ndarray
    gy: np.ndarray
    gz: np.ndarray
    voxel: np.ndarray
    case: np.ndarray
    misses: int = 0                   # requested gates no direction could place

    def counts(self) -> Dict[str, int]:
        return {c: int(np.count_nonzero(self.case == c)) for c in CASES}

    def __len__(self) -> int:
        return int(self.gx.shape[0])


def voxel_centres(grid_shape, grid_limits) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    nz, ny, nx = grid_shape
    return (axis_coords_f32(grid_limits[0][0], grid_limits[0][1], nz), axis_coords_f32(grid_limits[1][0], grid_limits[1][1], ny),
            axis_coords_f32(grid_limits[2][0], grid_limits[2][1], nx))


def rim_cloud(grid_shape, grid_limits, min_radius: float, beam_factor: float, seed: int,
              cases: Sequence[str] = CASES, per_voxel: Sequence[int] = (0, 1, 1, 2, 2, 3, 3),
              voxels: Optional[Sequence[int]] = None, outward: bool = False) -> RimCloud:
    """Plant gates on the rims of the chosen voxels (default: every voxel of the grid).

    Each voxel gets ``rng.choice(per_voxel)`` gates, each of a case drawn from ``cases`` (D only where voxel and radius
    are integers; a voxel where a case cannot be planted gets another one).  ``outward``: the gates of voxels on a face of
    the grid point out of the grid across that face (beyond its x / y / z extent)."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = grid_shape
    zc, yc, xc = voxel_centres(grid_shape, grid_limits)
    if voxels is None:
        voxels = range(nz * ny * nx)
    pts, vox, lab = [], [], []
    misses = 0
    for v in voxels:
        iz, rem = divmod(int(v), ny * nx)
        iy, ix = divmod(rem, nx)
        rim = voxel_rim(xc[ix], yc[iy], zc[iz], min_radius, beam_factor)
        direction = None
        if outward:
            spec = "".join("-" if i == 0 and n > 1 else "+" if i == n - 1 and n > 1 else "."
                           for i, n in ((ix, nx), (iy, ny), (iz, nz)))
            direction = None if spec == "..." else "out:" + spec
        for _ in range(int(rng.choice(per_voxel))):
            want = [str(c) for c in rng.permutation(list(cases))]
            for case in want:
                g = plant(rim, case, rng, direction=direction)
                if g is not None:
                    break
            else:
                misses += 1
                continue
            pts.append(g); vox.append(v); lab.append(case)
    p = np.array(pts, dtype=np.float32).reshape(-1, 3)
    return RimCloud(p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy(), np.array(vox, dtype=np.int64),
                    np.array(lab, dtype="<U1"), misses)


def point_cloud(xs, ys, zc, min_radius: float, beam_factor: float, seed: int,
                per_sample: Sequence[int] = (0, 1, 1, 2, 2, 3, 3), cases: Sequence[str] = CASES, direction=None) -> RimCloud:
    """Plant gates on the rims of the samples ``(xs[i], ys[i], zc[k])`` of a section: points anywhere, no lattice.

    As :func:`rim_cloud` per sample: ``rng.choice(per_sample)`` gates, each of a case drawn from ``cases`` (a sample where
    a case cannot be planted gets another one).  ``direction``: None, one ``'out:<signs>'`` spec for every point, or a
    sequence with one spec (or None) per point.  ``voxel`` of the result is the sample's row ``k * len(xs) + i``, the row
    order of a section."""
    rng = np.random.default_rng(seed)
    xs = np.asarray(xs, dtype=np.float32)
    ys = np.asarray(ys, dtype=np.float32)
    zc = np.asarray(zc, dtype=np.float32)
    n = xs.shape[0]
    per_point = [direction] * n if direction is None or isinstance(direction, str) else list(direction)
    if len(per_point) != n:
        raise ValueError(f"{len(per_point)} directions for {n} points")
    pts, vox, lab = [], [], []
    misses = 0
    for k in range(zc.shape[0]):
        for i in range(n):
            rim = voxel_rim(xs[i], ys[i], zc[k], min_radius, beam_factor)
            for _ in range(int(rng.choice(per_sample))):
                want = [str(c) for c in rng.permutation(list(cases))]
                for case in want:
                    g = plant(rim, case, rng, direction=per_point[i])
                    if g is not None:
                        break
                else:
                    misses += 1
                    continue
                pts.append(g); vox.append(k * n + i); lab.append(case)
    p = np.array(pts, dtype=np.float32).reshape(-1, 3)
    return RimCloud(p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy(), np.array(vox, dtype=np.int64),
                    np.array(lab, dtype="<U1"), misses)


def vertical_cloud(grid_shape, grid_limits, min_radius: float, beam_factor: float, voxels: Sequence[int]) -> RimCloud:
    """For voxels on the radar's vertical (x = y = 0): the innermost gate inside and the outermost gate outside the rim,
    straight above and straight below (the tightest case of the per-level lists' reach bound)."""
    rng = np.random.default_rng(0)
    nz, ny, nx = grid_shape
    zc, yc, xc = voxel_centres(grid_shape, grid_limits)
    pts, vox, lab = [], [], []
    for v in voxels:
        iz, rem = divmod(int(v), ny * nx)
        iy, ix = divmod(rem, nx)
        rim = voxel_rim(xc[ix], yc[iy], zc[iz], min_radius, beam_factor)
        for d in ("up", "down"):
            for side in ("<", ">"):
                g = plant(rim, side, rng, direction=d)
                if g is None:
                    raise ValueError(f"voxel {v}: no {d} gate {side} the rim")
                pts.append(g); vox.append(v)
                lab.append(classify(g[0:1], g[1:2], g[2:3], rim)[0])
    p = np.array(pts, dtype=np.float32).reshape(-1, 3)
    return RimCloud(p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy(), np.array(vox, dtype=np.int64), np.array(lab, dtype="<U1"))


def relabel(cloud: RimCloud, grid_shape, grid_limits, min_radius: float, beam_factor: float) -> np.ndarray:
    """Recompute every planted gate's label against its voxel from scratch (for checks)."""
    nz, ny, nx = grid_shape
    zc, yc, xc = voxel_centres(grid_shape, grid_limits)
    out = np.empty(len(cloud), dtype="<U1")
    for i, v in enumerate(cloud.voxel):
        iz, rem = divmod(int(v), ny * nx)
        iy, ix = divmod(rem, nx)
        rim = voxel_rim(xc[ix], yc[iy], zc[iz], min_radius, beam_factor)
        out[i] = classify(cloud.gx[i:i + 1], cloud.gy[i:i + 1], cloud.gz[i:i + 1], rim)[0]
    return out


# --------------------------------------------------------------------------------------------------
# the CSR-free gridder's float32 weights (grid mode of roi_block_kernel), emulated per pair
# --------------------------------------------------------------------------------------------------
def k2_weights_f32(pairs: dict, weighting: str, cressman_numerator: str = "f64") -> np.ndarray:
    """The float32 weight grid mode multiplies with, for every pair of ``pairs`` (radar_grid_oracle.pair_geometry):

    * barnes2: ``exp2f(d2f * inv_r2q) + 1e-5f`` with ``inv_r2q = (float)(-log2(e) * 4 / r2)``, d2f as :func:`d2f_kernel`
      and exp2 rounded correctly (the hardware's v_exp_f32 may differ by an ulp);
    * cressman: ``(float)(r2 - d2) / (r2f + d2f)``, numerator from the float64 d2; ``cressman_numerator='f32'`` gives the
      all-float32 ``(r2f - d2f) / (r2f + d2f)`` the kernel used before, whose numerator cancels at the rim;
    * nearest: 1."""
    n = pairs["d2"].shape[0]
    if weighting == "nearest":
        return np.ones(n, dtype=np.float32)
    d2f = d2f_kernel(pairs["gx"], pairs["gy"], pairs["gz"], pairs["vx"], pairs["vy"], pairs["vz"])
    r2 = pairs["r2"]
    r2f = r2.astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if weighting == "barnes2":
            inv_r2q = (-1.4426950408889634 * 4.0 / r2).astype(np.float32)
            t = (d2f * inv_r2q).astype(np.float32)
            return (np.exp2(t.astype(np.float64)).astype(np.float32) + _F32(1e-5)).astype(np.float32)
        if weighting == "cressman":
            num = (r2 - pairs["d2"]).astype(np.float32) if cressman_numerator == "f64" else (r2f - d2f).astype(np.float32)
            return (num / (r2f + d2f).astype(np.float32)).astype(np.float32)
    raise ValueError(weighting)
