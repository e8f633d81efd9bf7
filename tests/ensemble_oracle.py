"""Probabilistic nowcasts restated in NumPy for the tests of ``radar_processor_amd/ensemble.py`` and ``csrc/rg_ensemble.hip``
-- written from the formulas of ``include/radargrid_ensemble.h``, never from either.  The steps shared with the advection (the
source position and the two sampling rules) are those of ``tests/motion_oracle.py``.

* :func:`member_samples`: float32 ``[M, h, w]``, every member's sample of one lead (NaN = missing);
* :func:`exceedance`: ``prob``, ``counts``, ``members`` and ``mean`` of all leads;
* :func:`weight_sums`: the bilinear rule's float64 weight sum per member and pixel (what decides "missing" next to a hole);
* :func:`histogram`: ``hist`` and ``valid`` of ``rg_ensemble_histogram_u8``;
* :func:`brier_direct` and friends: the scores formed pixel by pixel, for ``probability_scores``.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import motion_oracle as mo

NAN32 = np.float32(np.nan)


class Exceedance(NamedTuple):
    prob: np.ndarray        # float32 [L, T, h, w]
    counts: np.ndarray      # uint8 [L, T, h, w]
    members: np.ndarray     # uint8 [L, h, w]
    mean: np.ndarray        # float32 [L, h, w]


def _positions(src, motion, lat, lead, shifts_l, substeps):
    """``(fy, fx)`` float64 ``[M, h, w]``: step 1 (b = p - d) and step 2 (b - shift) of the header."""
    by, bx = mo.source_position(src.shape, motion, lat, lead, substeps)
    s = np.asarray(shifts_l, dtype=np.float64)
    return by[None] - s[:, 0, None, None], bx[None] - s[:, 1, None, None]


def member_samples(src, motion, lat, lead, shifts_l, substeps=1, method="nearest") -> np.ndarray:
    src = np.ascontiguousarray(src, dtype=np.float32)
    fy, fx = _positions(src, motion, lat, lead, shifts_l, substeps)
    rule = mo.sample_nearest if method == "nearest" else mo.sample_bilinear
    with np.errstate(invalid="ignore"):
        return np.stack([rule(src[None], fy[m], fx[m], np.nan)[0] for m in range(fy.shape[0])])


def weight_sums(src, motion, lat, lead, shifts_l, substeps=1) -> np.ndarray:
    """float64 ``[M, h, w]``: the sum of the weights of the taps that lie inside the plane and are not NaN."""
    src = np.ascontiguousarray(src, dtype=np.float32)
    h, w = src.shape
    fy, fx = _positions(src, motion, lat, lead, shifts_l, substeps)
    y0, x0 = np.floor(fy), np.floor(fx)
    ty, tx = fy - y0, fx - x0
    wsum = np.zeros_like(fy)
    for (oy, ox), wt in zip(((0, 0), (0, 1), (1, 0), (1, 1)), ((1.0 - ty) * (1.0 - tx), (1.0 - ty) * tx, ty * (1.0 - tx), ty * tx)):
        yy, xx = y0 + oy, x0 + ox
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        v = src[np.where(ok, yy, 0).astype(np.int64), np.where(ok, xx, 0).astype(np.int64)]
        wsum = wsum + np.where(ok & ~np.isnan(v), wt, 0.0)
    return wsum


def reduce_members(samples, thresholds, min_members=1):
    """Steps 3 .. 5 and the outputs for ONE lead: ``samples`` float32 ``[M, h, w]`` -> ``(prob [T, h, w], counts, members, mean)``."""
    thr = np.asarray(thresholds, dtype=np.float32)
    present = ~np.isnan(samples)
    n_valid = present.sum(axis=0)
    with np.errstate(invalid="ignore"):
        counts = np.stack([(present & (samples >= t)).sum(axis=0) for t in thr])
    total = np.zeros(samples.shape[1:], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for m in range(samples.shape[0]):                                    # ascending m, one float64 add per present member
            total = np.where(present[m], total + samples[m].astype(np.float64), total)
    enough = n_valid >= min_members
    den = np.where(enough, n_valid, 1).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        prob = np.where(enough[None], (counts.astype(np.float64) / den[None]).astype(np.float32), NAN32)
        mean = np.where(enough, (total / den).astype(np.float32), NAN32)
    return prob.astype(np.float32), counts.astype(np.uint8), n_valid.astype(np.uint8), mean.astype(np.float32)


def exceedance(src, motion, lat, leads, shifts, thresholds, substeps=1, method="nearest", min_members=1) -> Exceedance:
    h, w = np.shape(src)
    L, T = len(leads), len(thresholds)
    out = Exceedance(np.empty((L, T, h, w), np.float32), np.empty((L, T, h, w), np.uint8), np.empty((L, h, w), np.uint8),
                     np.empty((L, h, w), np.float32))
    for l, lead in enumerate(leads):
        out.prob[l], out.counts[l], out.members[l], out.mean[l] = reduce_members(
            member_samples(src, motion, lat, lead, shifts[l], substeps, method), thresholds, min_members)
    return out


def histogram(counts, members, obs, mask, n_members, thresholds):
    """``(hist int64 [n, T, M + 1, 2], valid int64 [n])``."""
    counts, members, obs = np.asarray(counts), np.asarray(members), np.asarray(obs, dtype=np.float32)
    thr = np.asarray(thresholds, dtype=np.float32)
    n, T = counts.shape[:2]
    M = int(n_members)
    ok = ~np.isnan(obs) & (members == M) & (counts <= M).all(axis=1)
    if mask is not None:
        ok &= np.asarray(mask) == 0
    hist = np.zeros((n, T, M + 1, 2), dtype=np.int64)
    for p in range(n):
        sel = ok[p]
        for t in range(T):
            k = counts[p, t][sel].astype(np.int64)
            with np.errstate(invalid="ignore"):
                o = (obs[p][sel] >= thr[t]).astype(np.int64)
            hist[p, t] = np.bincount(k * 2 + o, minlength=2 * (M + 1)).reshape(M + 1, 2)
    return hist, ok.reshape(n, -1).sum(axis=1).astype(np.int64)


# ---- the scores, pixel by pixel ------------------------------------------------------------------------------------------------
def brier_direct(k, o, n_members) -> float:
    """``mean((k / M - o)^2)`` over pixels: ``k`` integer counts, ``o`` 0 / 1."""
    p = np.asarray(k, dtype=np.float64) / float(n_members)
    return float(np.mean((p - np.asarray(o, dtype=np.float64)) ** 2))


def table_from_pixels(k, o, n_members) -> np.ndarray:
    """int64 ``[1, 1, M + 1, 2]`` from flat integer ``k`` and 0 / 1 ``o``."""
    flat = np.asarray(k, dtype=np.int64) * 2 + np.asarray(o, dtype=np.int64)
    return np.bincount(flat, minlength=2 * (n_members + 1)).reshape(1, 1, n_members + 1, 2)
