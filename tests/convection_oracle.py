"""NumPy restatement of the convective / stratiform contract (include/radargrid_hip.h, "Convective / stratiform
classification"): echo, the fixed-point linear reflectivity q, footprint sums by row ``cumsum``s and shifted differences in
int64, the background, the convective centres and the convective area -- and, beside it, the DIRECT definition, which loops
over every offset of the footprint and uses no prefix.

Every function takes ``q`` (or the stage before it) as an optional input, so that a test can hand it the device's: the only
place where the device may differ from NumPy is one unit of ``q`` at a rounding tie of ``exp10``, and one float32 step of
``log10`` in the background."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

Q_ONE = 65536.0
STEINER = (10.0, 180.0)


def as3(a: np.ndarray) -> np.ndarray:
    return a[None] if a.ndim == 2 else a


def echo(dbz: np.ndarray, mask: Optional[np.ndarray] = None, min_dbz: float = 5.0) -> np.ndarray:
    """bool: not NaN, mask 0, ``dBZ >= min_dbz`` in float32."""
    with np.errstate(invalid="ignore"):
        out = ~np.isnan(dbz) & (dbz >= np.float32(min_dbz))
    return out if mask is None else out & (mask == 0)


def quantize(dbz: np.ndarray, mask: Optional[np.ndarray] = None, min_dbz: float = 5.0) -> np.ndarray:
    """int64 ``q = rint(65536 * 10^(clamp(dBZ, -10, 80) / 10))`` on echo pixels, 0 elsewhere."""
    e = echo(dbz, mask, min_dbz)
    v = np.clip(np.where(e, dbz, np.float32(0.0)).astype(np.float64), -10.0, 80.0)
    return np.where(e, np.rint(Q_ONE * np.power(10.0, v / 10.0)).astype(np.int64), np.int64(0))


def _shift_diff(prefix: np.ndarray, half: int) -> np.ndarray:
    """``prefix`` ``[..., w + 1]`` exclusive along x -> the sum over columns ``x - half .. x + half`` cut to the plane."""
    w = prefix.shape[-1] - 1
    x = np.arange(w)
    return prefix[..., np.minimum(x + half, w - 1) + 1] - prefix[..., np.maximum(x - half, 0)]


def footprint_sum(values: np.ndarray, hw: Sequence[int]) -> np.ndarray:
    """int64 ``[n, h, w]``: the sum of the integer planes ``values`` over the footprint ``hw[0 .. ry]`` at every pixel, by row
    prefixes and shifted differences."""
    values = as3(np.asarray(values)).astype(np.int64)
    n, h, w = values.shape
    prefix = np.zeros((n, h, w + 1), dtype=np.int64)
    np.cumsum(values, axis=2, out=prefix[..., 1:])
    out = np.zeros((n, h, w), dtype=np.int64)
    for d, half in enumerate(hw):
        rows = _shift_diff(prefix, int(half))                          # the row sums of this half-width, for every row
        for dy in ((0,) if d == 0 else (-d, d)):
            lo, hi = max(0, -dy), min(h, h - dy)                        # output rows y with 0 <= y + dy < h
            if lo < hi:
                out[:, lo:hi] += rows[:, lo + dy:hi + dy]
    return out


def footprint_sum_direct(values: np.ndarray, hw: Sequence[int]) -> np.ndarray:
    """The same by the definition, without a prefix: for every offset ``(dy, dx)`` of the footprint, every pixel takes the
    value at ``(y + dy, x + dx)`` where that lies in the plane."""
    values = as3(np.asarray(values)).astype(np.int64)
    n, h, w = values.shape
    ry = len(hw) - 1
    out = np.zeros((n, h, w), dtype=np.int64)
    for dy in range(-min(ry, h - 1), min(ry, h - 1) + 1):
        half = min(int(hw[abs(dy)]), w - 1)
        y_lo, y_hi = max(0, -dy), min(h, h - dy)
        for dx in range(-half, half + 1):
            x_lo, x_hi = max(0, -dx), min(w, w - dx)
            out[:, y_lo:y_hi, x_lo:x_hi] += values[:, y_lo + dy:y_hi + dy, x_lo + dx:x_hi + dx]
    return out


def footprint_area(shape, hw: Sequence[int]) -> np.ndarray:
    """int64 ``[h, w]``: the number of pixels of the footprint at every pixel that lie in the plane -- the footprint sum of a
    plane of ones in closed form, row span by row span, without a prefix."""
    h, w = shape
    ry = len(hw) - 1
    x = np.arange(w)
    out = np.zeros((h, w), dtype=np.int64)
    for y in range(h):
        for r in range(max(y - ry, 0), min(y + ry, h - 1) + 1):
            half = int(hw[abs(r - y)])
            out[y] += np.minimum(x + half, w - 1) - np.maximum(x - half, 0) + 1
    return out


def background_from_sums(S: np.ndarray, N: np.ndarray) -> np.ndarray:
    """float32 ``10 * log10(S / N / 65536)`` in float64, NaN where ``N == 0``."""
    with np.errstate(invalid="ignore", divide="ignore"):
        value = 10.0 * np.log10(S.astype(np.float64) / N.astype(np.float64) / Q_ONE)
    return np.where(N > 0, value, np.nan).astype(np.float32)


def background(dbz, hw, mask=None, min_dbz: float = 5.0, q: Optional[np.ndarray] = None, direct: bool = False):
    """``(S int64, N int32, bkg float32)`` of shape ``[n, h, w]``; ``q`` replaces NumPy's own quantisation."""
    dbz = as3(dbz)
    mask = None if mask is None else as3(mask)
    q = quantize(dbz, mask, min_dbz) if q is None else as3(q)
    total = footprint_sum_direct if direct else footprint_sum
    S, N = total(q, hw), total(echo(dbz, mask, min_dbz), hw).astype(np.int32)
    return S, N, background_from_sums(S, N)


def peak_delta(b: np.ndarray, peak=STEINER) -> np.ndarray:
    """float64: ``peak_a`` for ``b < 0``, otherwise ``peak_a - b * b / peak_b`` where that is positive, else 0."""
    b = np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        curve = peak[0] - b * b / peak[1]
        return np.where(b < 0.0, peak[0], np.where(curve > 0.0, curve, 0.0))


def centres(dbz, bkg, edges: Sequence[float], mask=None, min_dbz: float = 5.0, intense: float = 40.0, peak=STEINER,
            return_criteria: bool = False):
    """uint8: 0, or the class ``1 + #{e : b >= e}`` of the centre; float64 on the float32 ``dbz`` and ``bkg``."""
    e = echo(dbz, mask, min_dbz)
    v, b = dbz.astype(np.float64), bkg.astype(np.float64)
    with np.errstate(invalid="ignore"):
        by_intensity = e & (v >= float(intense))
        by_peak = e & ((v - b) >= peak_delta(b, peak))
        k = 1 + sum((b >= float(edge)).astype(np.uint8) for edge in edges) if len(edges) else np.ones(b.shape, np.uint8)
    out = np.where(by_intensity | by_peak, k, 0).astype(np.uint8)
    return (out, by_intensity, by_peak) if return_criteria else out


def area(centre_plane, dbz, footprints: Sequence[Sequence[int]], mask=None, min_dbz: float = 5.0, direct: bool = False):
    """uint8: 0 no echo, 2 an echo pixel with a centre of class ``k`` inside footprint ``k`` around it, 1 any other echo."""
    centre_plane, dbz = as3(centre_plane), as3(dbz)
    e = echo(dbz, None if mask is None else as3(mask), min_dbz)
    total = footprint_sum_direct if direct else footprint_sum
    near = np.zeros(dbz.shape, dtype=bool)
    for k, hw in enumerate(footprints, start=1):
        near |= total(centre_plane == k, hw) > 0
    return np.where(e, np.where(near, 2, 1), 0).astype(np.uint8)


def classify(dbz, hw, footprints, edges, mask=None, min_dbz: float = 5.0, intense: float = 40.0, peak=STEINER,
             q: Optional[np.ndarray] = None, direct: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(classes, bkg, centres)`` of shape ``[n, h, w]``: the whole chain."""
    dbz = as3(dbz)
    mask = None if mask is None else as3(mask)
    _, _, bkg = background(dbz, hw, mask, min_dbz, q, direct)
    c = centres(dbz, bkg, edges, mask, min_dbz, intense, peak)
    return area(c, dbz, footprints, mask, min_dbz, direct), bkg, c


def disk_footprint_brute(radius_m: float, dy: float, dx: float) -> Tuple[int, ...]:
    """The footprint of a disk by testing every offset up to 128 pixels: ``(k dx)^2 <= R^2 - (d dy)^2`` in float64."""
    d = np.arange(0, 129, dtype=np.float64)
    left = radius_m * radius_m - (d * dy) * (d * dy)                                      # per row distance
    inside = ((d * dx) * (d * dx))[None, :] <= left[:, None]                              # [dy index, dx index]
    rows = np.flatnonzero((d * dy) * (d * dy) <= radius_m * radius_m)
    return tuple(int(np.flatnonzero(inside[r]).max()) for r in rows)
