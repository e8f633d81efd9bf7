"""Echo motion and nowcasts restated in NumPy for the tests of ``radar_processor_amd/motion.py`` and ``csrc/rg_motion.hip``
-- written from the formulas of ``include/radargrid_hip.h`` ("Echo motion and nowcasts"), never from either.

* :func:`quantize`: float32 planes to 8-bit levels, in float32 like the header;
* :func:`block_match`: int64 sums and float64 scores for every block and candidate.  The sums over a block are taken from
  integral images (a sum of integers does not depend on how it is formed); :func:`block_scores_direct` forms them literally,
  one block at a time, and tests/test_motion_oracle.py holds the two against each other;
* :func:`fill_motion`: the replacement of missing or poorly correlated vectors;
* :func:`advect`: the float64 displacement and the two sampling rules;
* :func:`nowcast`: the chain.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

KEY_SHIFT = 13                          # tie key = (dy*dy + dx*dx) << 13 | candidate index; 65 * 65 < 2^13


class Lattice(NamedTuple):              # field for field the rg_motion_lattice
    origin_y: float
    origin_x: float
    step_y: float
    step_x: float
    ny: int
    nx: int


class Match(NamedTuple):
    disp: np.ndarray                    # int16 [n, nby, nbx, 2]
    motion: np.ndarray                  # float64 [n, nby, nbx, 2] BEFORE the rounding to float32; NaN: no vector
    score: np.ndarray                   # float64 [n, nby, nbx]
    scores: np.ndarray                  # float64 [n, nby, nbx, 2R+1, 2R+1]: every candidate, NaN where it is not qualified
    valid: np.ndarray                   # bool [n, nby, nbx]: enough echo and va > 0


def block_lattice(shape, B, S) -> Lattice:
    h, w = shape
    return Lattice((B - 1) / 2.0, (B - 1) / 2.0, float(S), float(S), (h - B) // S + 1, (w - B) // S + 1)


# ---- quantise ----------------------------------------------------------------------------------------------------------------
def quantize(src, lo=0.0, hi=63.5, mask=None) -> np.ndarray:
    lo32 = np.float32(lo)
    inv = np.float32(254.0 / (float(hi) - float(lo)))
    v = np.asarray(src, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (v - lo32) * inv                                            # two float32 operations
        echo = v >= lo32                                                # false for NaN and -inf
        if mask is not None:
            echo &= np.asarray(mask) == 0
        capped = echo & (t >= np.float32(254.0))
        trunc = np.where(echo & ~capped, t, np.float32(0.0)).astype(np.int64)       # (int)t: towards zero, t >= 0 here
    return np.where(echo, 1 + np.where(capped, 254, trunc), 0).astype(np.uint8)


# ---- block match -------------------------------------------------------------------------------------------------------------
def _integral(a):
    out = np.zeros((a.shape[0] + 1, a.shape[1] + 1), dtype=np.int64)
    out[1:, 1:] = a.cumsum(axis=0).cumsum(axis=1)
    return out


def _boxes(integral, ys, xs, B):
    """Sums over the B x B boxes whose first pixel is (ys[j], xs[i])."""
    return (integral[ys + B][:, xs + B] - integral[ys][:, xs + B] - integral[ys + B][:, xs] + integral[ys][:, xs])


def _ncc(N, sa, saa, sb, sbb, sab):
    """The header's score from int64 sums (arrays); NaN where va or vb is not positive."""
    va, vb = N * saa - sa * sa, N * sbb - sb * sb
    ok = (va > 0) & (vb > 0)
    num = (N * sab - sa * sb).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = num / np.sqrt(va.astype(np.float64) * vb.astype(np.float64))
    return np.where(ok, s, np.nan)


def _pair_scores(prev, nxt, B, S, R, min_echo):
    h, w = prev.shape
    a, b = prev.astype(np.int64), nxt.astype(np.int64)
    N = B * B
    ys, xs = np.arange((h - B) // S + 1) * S, np.arange((w - B) // S + 1) * S
    sa, saa = _boxes(_integral(a), ys, xs, B), _boxes(_integral(a * a), ys, xs, B)
    echo = _boxes(_integral((a != 0).astype(np.int64)), ys, xs, B)
    valid = (echo >= min_echo) & (N * saa - sa * sa > 0)
    ib, ibb = _integral(b), _integral(b * b)
    side = 2 * R + 1
    scores = np.full((len(ys), len(xs), side, side), np.nan)
    for dy in range(-R, R + 1):
        oky = (ys + dy >= 0) & (ys + dy + B <= h)
        for dx in range(-R, R + 1):
            okx = (xs + dx >= 0) & (xs + dx + B <= w)
            if not (oky.any() and okx.any()):
                continue
            prod = np.zeros((h, w), dtype=np.int64)                     # a[y, x] * b[y + dy, x + dx] where both exist
            y_lo, y_hi, x_lo, x_hi = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
            prod[y_lo:y_hi, x_lo:x_hi] = a[y_lo:y_hi, x_lo:x_hi] * b[y_lo + dy:y_hi + dy, x_lo + dx:x_hi + dx]
            yb, xb = np.where(oky, ys + dy, 0), np.where(okx, xs + dx, 0)
            s = _ncc(N, sa, saa, _boxes(ib, yb, xb, B), _boxes(ibb, yb, xb, B), _boxes(_integral(prod), ys, xs, B))
            scores[:, :, dy + R, dx + R] = np.where(valid & oky[:, None] & okx[None, :], s, np.nan)
    return scores, valid


def block_scores_direct(prev, nxt, by, bx, B, S, R):
    """The scores of ONE block formed literally: ``(float64 [2R+1, 2R+1] with NaN where unqualified, echo pixels, va)``."""
    h, w = prev.shape
    y0, x0, N = by * S, bx * S, B * B
    a = prev[y0:y0 + B, x0:x0 + B].astype(np.int64)
    sa, saa = int(a.sum()), int((a * a).sum())
    va = N * saa - sa * sa
    out = np.full((2 * R + 1, 2 * R + 1), np.nan)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if y0 + dy < 0 or y0 + dy + B > h or x0 + dx < 0 or x0 + dx + B > w:
                continue
            b = nxt[y0 + dy:y0 + dy + B, x0 + dx:x0 + dx + B].astype(np.int64)
            sb, sbb, sab = int(b.sum()), int((b * b).sum()), int((a * b).sum())
            vb = N * sbb - sb * sb
            if va > 0 and vb > 0:
                out[dy + R, dx + R] = np.float64(N * sab - sa * sb) / np.sqrt(np.float64(va) * np.float64(vb))
    return out, int((a != 0).sum()), va


def _offset(scores, cy, cx, axis, s0):
    """The parabola of the header along one axis of a block's score table."""
    side = scores.shape[0]
    c = cy if axis == 0 else cx
    if c == 0 or c == side - 1:
        return 0.0
    m = scores[cy - 1, cx] if axis == 0 else scores[cy, cx - 1]
    p = scores[cy + 1, cx] if axis == 0 else scores[cy, cx + 1]
    if np.isnan(m) or np.isnan(p):
        return 0.0
    den = m - 2.0 * s0 + p
    if not den < 0.0:
        return 0.0
    return float(min(max(0.5 * (m - p) / den, -0.5), 0.5))


def block_match(prev, nxt, B, S, R, min_echo=None) -> Match:
    """``prev`` / ``nxt``: uint8 levels ``[h, w]`` or ``[n, h, w]``; always returns the leading axis."""
    prev, nxt = np.asarray(prev), np.asarray(nxt)
    if prev.ndim == 2:
        prev, nxt = prev[None], nxt[None]
    min_echo = B * B // 8 if min_echo is None else min_echo
    n, (h, w) = prev.shape[0], prev.shape[1:]
    nby, nbx, side = (h - B) // S + 1, (w - B) // S + 1, 2 * R + 1
    disp = np.zeros((n, nby, nbx, 2), dtype=np.int16)
    motion = np.full((n, nby, nbx, 2), np.nan)
    score = np.full((n, nby, nbx), np.nan)
    scores = np.empty((n, nby, nbx, side, side))
    valid = np.empty((n, nby, nbx), dtype=bool)
    cy_all, cx_all = np.divmod(np.arange(side * side), side)
    key = (((cy_all - R) ** 2 + (cx_all - R) ** 2) << KEY_SHIFT) | np.arange(side * side)
    for k in range(n):
        scores[k], valid[k] = _pair_scores(prev[k], nxt[k], B, S, R, min_echo)
        flat = scores[k].reshape(nby, nbx, -1)
        for by in range(nby):
            for bx in range(nbx):
                have = ~np.isnan(flat[by, bx])
                if not have.any():
                    continue
                s0 = flat[by, bx][have].max()
                c = int(key[have & (flat[by, bx] == s0)].min()) & ((1 << KEY_SHIFT) - 1)    # the full tie key
                cy, cx = divmod(c, side)
                disp[k, by, bx] = (cy - R, cx - R)
                motion[k, by, bx] = ((cy - R) + _offset(scores[k, by, bx], cy, cx, 0, s0),
                                     (cx - R) + _offset(scores[k, by, bx], cy, cx, 1, s0))
                score[k, by, bx] = s0
    return Match(disp, motion, score, scores, valid)


# ---- fill --------------------------------------------------------------------------------------------------------------------
def fill_motion(motion, score, min_score=0.5) -> np.ndarray:
    """float32 ``[nby, nbx, 2]`` and ``[nby, nbx]`` of ONE pair -> the filled float32 field."""
    motion, score = np.asarray(motion, dtype=np.float32), np.asarray(score, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        good = (score >= np.float32(min_score)) & ~np.isnan(motion).any(axis=-1)
    count = int(good.sum())
    total = np.where(good[..., None], motion.astype(np.float64), 0.0).sum(axis=(0, 1))
    mean = (total / count if count else np.zeros(2)).astype(np.float32)
    return np.where(good[..., None], motion, mean[None, None, :])


# ---- advect ------------------------------------------------------------------------------------------------------------------
def motion_at(motion, lat: Lattice, py, px):
    """``(Vy, Vx)`` float64 at the float64 positions ``py``, ``px`` (arrays of one shape)."""
    def axis(p, origin, step, n):
        l = np.clip((p - origin) / step, 0.0, float(n - 1))
        j0 = np.minimum(np.floor(l), float(max(n - 2, 0))).astype(np.int64)
        return j0, np.minimum(j0 + 1, n - 1), l - j0

    j0, j1, ty = axis(py, lat.origin_y, lat.step_y, lat.ny)
    i0, i1, tx = axis(px, lat.origin_x, lat.step_x, lat.nx)
    m = np.asarray(motion, dtype=np.float32).astype(np.float64)
    out = []
    for comp in (0, 1):
        v = m[..., comp]
        out.append((v[j0, i0] * (1.0 - tx) + v[j0, i1] * tx) * (1.0 - ty) + (v[j1, i0] * (1.0 - tx) + v[j1, i1] * tx) * ty)
    return out[0], out[1]


def source_position(shape, motion, lat: Lattice, lead, substeps):
    """``(fy, fx)`` float64 ``[h, w]``: where every pixel's value comes from after ``lead`` intervals."""
    h, w = shape
    py, px = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    dy, dx = np.zeros((h, w)), np.zeros((h, w))
    dt = float(lead) / float(substeps)
    for _ in range(substeps):
        vy, vx = motion_at(motion, lat, py - dy, px - dx)
        dy, dx = dy + dt * vy, dx + dt * vx
    return py - dy, px - dx


def sample_nearest(src, fy, fx, fill):
    """float32 ``[P, h, w]`` -> ``[P, h, w]``, bits copied."""
    h, w = src.shape[-2:]
    iy, ix = np.floor(fy + 0.5), np.floor(fx + 0.5)
    inside = (iy >= 0) & (iy < h) & (ix >= 0) & (ix < w)
    bits = src.view(np.uint32)[:, np.where(inside, iy, 0).astype(np.int64), np.where(inside, ix, 0).astype(np.int64)]
    return np.where(inside[None], bits, np.float32(fill).reshape(1).view(np.uint32)[0]).view(np.float32)


def sample_bilinear(src, fy, fx, fill):
    """float32 ``[P, h, w]`` -> float32 ``[P, h, w]``: ``(float)(vsum / wsum)`` where wsum >= 0.5, else ``fill``."""
    h, w = src.shape[-2:]
    y0, x0 = np.floor(fy), np.floor(fx)
    ty, tx = fy - y0, fx - x0
    weights = ((1.0 - ty) * (1.0 - tx), (1.0 - ty) * tx, ty * (1.0 - tx), ty * tx)
    out = np.empty(src.shape, dtype=np.float32)
    for p in range(src.shape[0]):
        wsum, vsum = np.zeros_like(fy), np.zeros_like(fy)
        for (oy, ox), wt in zip(((0, 0), (0, 1), (1, 0), (1, 1)), weights):
            yy, xx = y0 + oy, x0 + ox
            ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            v = src[p][np.where(ok, yy, 0).astype(np.int64), np.where(ok, xx, 0).astype(np.int64)].astype(np.float64)
            ok &= ~np.isnan(v)
            wsum = wsum + np.where(ok, wt, 0.0)
            with np.errstate(invalid="ignore"):                             # a weight of 0 times an infinite tap is NaN, as on the device
                vsum = vsum + np.where(ok, wt * np.where(ok, v, 0.0), 0.0)
        keep = wsum >= 0.5
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            out[p] = np.where(keep, (vsum / np.where(keep, wsum, 1.0)).astype(np.float32), np.float32(fill))
    return out


def advect(src, motion, lat: Lattice, leads, substeps=1, method="nearest", fill=np.nan) -> np.ndarray:
    """float32 ``[P, h, w]`` -> float32 ``[L, P, h, w]``."""
    src = np.ascontiguousarray(src, dtype=np.float32)
    out = np.empty((len(leads),) + src.shape, dtype=np.float32)
    for k, lead in enumerate(leads):
        fy, fx = source_position(src.shape[-2:], motion, lat, lead, substeps)
        out[k] = sample_nearest(src, fy, fx, fill) if method == "nearest" else sample_bilinear(src, fy, fx, fill)
    return out


# ---- the chain ---------------------------------------------------------------------------------------------------------------
def nowcast(prev, nxt, leads, B=32, S=16, R=16, lo=0.0, hi=63.5, min_echo=None, min_score=0.5, method="nearest", substeps=1,
            fill=np.nan):
    """``(forecast float32 [L, h, w], filled float32 motion [nby, nbx, 2], Match)`` of two float32 planes."""
    m = block_match(quantize(prev, lo, hi), quantize(nxt, lo, hi), B, S, R, min_echo)
    filled = fill_motion(m.motion[0].astype(np.float32), m.score[0].astype(np.float32), min_score)
    forecast = advect(np.asarray(nxt, dtype=np.float32)[None], filled, block_lattice(prev.shape, B, S), leads, substeps, method,
                      fill)
    return forecast[:, 0], filled, m
