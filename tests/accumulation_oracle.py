"""Rain rate and advection-corrected accumulation restated in NumPy for the tests of ``radar_processor_amd/accumulation.py``
and ``csrc/rg_accumulate.hip`` -- written from the formulas of ``include/radargrid_hip.h`` ("Rain rate and accumulation"),
never from either.  Positions and samples are those of ``tests/motion_oracle.py``.

* :func:`zr_constants`: the two doubles the host passes for ``Z = a R^b``;
* :func:`rain_rate`: dBZ planes to mm/h, float64 up to the one rounding to float32;
* :func:`accumulate`: the ``n_steps`` sub-instants of one interval, float64, in the header's order;
* :func:`accumulate_chain`: intervals summed as :class:`RainAccumulator` sums them.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

import motion_oracle as mo

MAX_ACC_STEPS = 64
NAN_BITS = 0x7FC00000


class Accumulation(NamedTuple):
    out: np.ndarray                     # float32 [P, h, w]
    steps: np.ndarray                   # uint8 [P, h, w]: the sub-instants that contributed
    both: int                           # how often each branch was taken, over all planes, pixels and steps
    only_prev: int
    only_next: int
    neither: int


def zr_constants(a=200.0, b=1.6):
    """``(p, q)`` with ``R = exp(dBZ * p - q)``."""
    return math.log(10.0) / (10.0 * float(b)), math.log(float(a)) / float(b)


def rain_rate(src, a=200.0, b=1.6, min_dbz=5.0, max_dbz=55.0, mask=None) -> np.ndarray:
    """float32 planes of any shape -> float32 mm/h of the same shape."""
    p, q = zr_constants(a, b)
    v = np.asarray(src, dtype=np.float32)
    v64 = v.astype(np.float64)
    none = np.isnan(v)
    if mask is not None:
        none = none | (np.asarray(mask) != 0)
    with np.errstate(invalid="ignore"):
        wet = v64 >= float(min_dbz)                                     # false for NaN and -inf
    c = np.minimum(np.where(wet, v64, float(min_dbz)), float(max_dbz))
    rate = np.exp(c * p - q).astype(np.float32)                         # multiply, subtract, exp: each rounded once
    out = np.where(wet, rate, np.float32(0.0)).astype(np.float32)
    out.view(np.uint32)[none] = NAN_BITS
    return out


def accumulate(rate_prev, rate_next, motion, lat: mo.Lattice, hours, n_steps, substeps=1, method="bilinear", min_steps=None,
               fill=np.nan) -> Accumulation:
    """float32 ``[P, h, w]`` twice -> :class:`Accumulation`."""
    prev = np.ascontiguousarray(rate_prev, dtype=np.float32)
    nxt = np.ascontiguousarray(rate_next, dtype=np.float32)
    assert prev.ndim == 3 and prev.shape == nxt.shape and 1 <= n_steps <= MAX_ACC_STEPS
    min_steps = n_steps if min_steps is None else min_steps
    shape = prev.shape[-2:]
    sample = mo.sample_nearest if method == "nearest" else mo.sample_bilinear
    total = np.zeros(prev.shape)
    n = np.zeros(prev.shape, dtype=np.int64)
    taken = [0, 0, 0, 0]
    for k in range(n_steps):
        s = (float(k) + 0.5) / float(n_steps)
        fy, fx = mo.source_position(shape, motion, lat, s, substeps)
        a = sample(prev, fy, fx, np.nan)
        fy, fx = mo.source_position(shape, motion, lat, s - 1.0, substeps)
        b = sample(nxt, fy, fx, np.nan)
        has_a, has_b = ~np.isnan(a), ~np.isnan(b)
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        with np.errstate(invalid="ignore"):
            blend = (1.0 - s) * np.where(has_a, a64, 0.0) + s * np.where(has_b, b64, 0.0)
        r = np.where(has_a & has_b, blend, np.where(has_a, a64, b64))
        present = has_a | has_b
        with np.errstate(invalid="ignore"):
            total = np.where(present, total + np.where(present, r, 0.0), total)
        n += present
        for slot, m in enumerate((has_a & has_b, has_a & ~has_b, ~has_a & has_b, ~present)):
            taken[slot] += int(m.sum())
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        depth = (float(hours) * (total / np.where(n > 0, n, 1).astype(np.float64))).astype(np.float32)
    out = np.where(n >= min_steps, depth, np.float32(fill)).astype(np.float32)
    fill_bits = np.float32(fill).reshape(1).view(np.uint32)[0]
    out.view(np.uint32)[n < min_steps] = fill_bits                     # the fill's own bits, a NaN's payload included
    return Accumulation(out, n.astype(np.uint8), *taken)


def trapezoid(rate_prev, rate_next, hours) -> np.ndarray:
    """float64: the trapezoid rule of the linear blend in time, where both ends are present."""
    return float(hours) * 0.5 * (np.asarray(rate_prev, dtype=np.float64) + np.asarray(rate_next, dtype=np.float64))


def window_total(intervals, end_times, now, window_seconds, skip_missing=False) -> np.ndarray:
    """What ``RainAccumulator.total`` returns: the float32 ``intervals`` whose end lies within ``window_seconds`` of ``now``,
    summed in float64 in time order and cast once; NaN propagates unless ``skip_missing`` (then a NaN adds nothing)."""
    total = None
    for plane, end in zip(intervals, end_times):
        if end <= now - window_seconds:
            continue
        v = np.asarray(plane, dtype=np.float32).astype(np.float64)
        if skip_missing:
            v = np.where(np.isnan(v), 0.0, v)
        total = v if total is None else total + v
    return None if total is None else total.astype(np.float32)
