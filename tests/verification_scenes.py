"""Scenes for the verification tests (tests/test_verification_scenes.py, tests/test_gpu_verification.py): a forecast and an
observation stack, an optional mask, thresholds and a ladder of window sizes.  Every scene and its restated result are
computed once, shared, and read-only.

The row pass of the summed-area table walks a row in trips of 64 pixels and carries the count from one trip to the next; the
sums kernel covers 256 pixels per workgroup and trip.  So the widths are 7 (less than a wavefront), 150 (three trips, the
carry crossed twice, no multiple of 4), 1 and 200 (single column, single row), 300 and 600."""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional, Tuple

import numpy as np

import verification_oracle as vo

WAVE = 64
ROWS_THRESHOLDS = (0.0, 7.5, 18.0, 25.25, 35.0, 45.0, 50.5, 60.0)
ROWS_LEVELS = (-np.inf, -5.0, -0.0, 0.0, 3.0, 7.5, 12.0, 18.0, 25.25, 30.0, 35.0, 45.0, 50.5, 55.0, 60.0, np.inf)
SCENES = ("rim", "rows", "line_h", "line_v", "none", "all", "big_sums", "many")


class Scene(NamedTuple):
    name: str
    forecast: np.ndarray                # float32 [n, h, w]
    observed: np.ndarray                # float32 [n, h, w]
    mask: Optional[np.ndarray]          # uint8 [n, h, w] or None
    thresholds: Tuple[float, ...]
    scales: Tuple[int, ...]


class Expected(NamedTuple):
    counts: np.ndarray                  # int64 [n, T, 3]
    valid: np.ndarray                   # int64 [n]
    sat_f: np.ndarray                   # int32 [n, T, h, w]
    sat_o: np.ndarray
    sums: np.ndarray                    # int64 [n, T, S, 3]


def levels(shape, seed, choices, nan_share=0.0):
    """float32 planes drawn from ``choices``; ``nan_share`` of the pixels NaN."""
    rng = np.random.default_rng(seed)
    out = np.asarray(choices, dtype=np.float32)[rng.integers(0, len(choices), shape)]
    if nan_share:
        out[rng.random(shape) < nan_share] = np.nan
    return out


def clipped_span(size, n):
    """int64 ``[size]``: how many of the ``n`` rows (columns) of the window at each position lie inside the plane."""
    at = np.arange(size)
    return (np.minimum(at - n // 2 + n - 1, size - 1) - np.maximum(at - n // 2, 0) + 1).astype(np.int64)


def sum_of_squared_areas(h, w, n) -> int:
    """The closed form of ``sum cf^2`` for a plane that exceeds everywhere: the window's clipped area factors into rows times
    columns, so the sum of its squares is the product of two one-dimensional sums.  A Python integer."""
    ry, rx = clipped_span(h, n), clipped_span(w, n)
    return int((ry * ry).sum()) * int((rx * rx).sum())


def _build(name: str) -> Scene:
    if name == "rim":                                     # windows cut by the border on every side; 255 covers the whole plane
        return Scene(name, levels((1, 5, 7), 3, (0.0, 20.0, 40.0)), levels((1, 5, 7), 4, (0.0, 20.0, 40.0)), None, (20.0,),
                     (1, 2, 3, 255))
    if name == "rows":
        shape = (3, 45, 150)
        rng = np.random.default_rng(11)
        mask = (rng.random(shape) < 0.03).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)
        return Scene(name, levels(shape, 5, ROWS_LEVELS, 0.05), levels(shape, 6, ROWS_LEVELS, 0.05), mask, ROWS_THRESHOLDS,
                     (1, 2, 3, 8, 31, 64, 255))
    if name in ("line_h", "line_v"):
        shape = (1, 1, 200) if name == "line_h" else (1, 200, 1)
        return Scene(name, levels(shape, 7, (5.0, 18.0, 35.0, 50.0), 0.03), levels(shape, 8, (5.0, 18.0, 35.0, 50.0), 0.03), None,
                     (18.0, 35.0), (1, 2, 3, 8, 64, 255))
    if name == "none":                                    # nothing exceeds: every sum 0, FSS NaN
        return Scene(name, levels((1, 45, 150), 9, (-np.inf, 0.0, 17.75)), levels((1, 45, 150), 10, (-np.inf, 0.0, 17.75)), None,
                     (18.0, 35.0), (1, 8, 255))
    if name == "all":                                     # everything exceeds: closed-form sums
        return Scene(name, levels((1, 45, 150), 12, (35.0, 40.0, np.inf)), levels((1, 45, 150), 13, (35.0, 40.0, np.inf)), None,
                     (18.0, 35.0), (1, 2, 8, 64, 255))
    if name == "big_sums":                                # cf^2 passes 2^31 at single pixels, the total passes 2^47
        return Scene(name, np.full((1, 300, 300), 50.0, np.float32), np.full((1, 300, 300), 1.0, np.float32), None, (35.0,), (255,))
    if name == "many":                                    # several workgroups per layer and scale, long columns
        shape = (2, 700, 600)
        rng = np.random.default_rng(17)
        forecast = rng.uniform(0.0, 60.0, shape).astype(np.float32)
        observed = np.where(rng.random(shape) < 0.7, forecast, rng.uniform(0.0, 60.0, shape)).astype(np.float32)
        forecast[rng.random(shape) < 0.01] = np.nan
        observed[rng.random(shape) < 0.01] = np.nan
        mask = np.zeros(shape, dtype=np.uint8)
        mask[:, 100:130, 500:590] = 1
        return Scene(name, forecast, observed, mask, (10.0, 25.0, 40.0, 55.0), (1, 16, 129))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def scene(name: str) -> Scene:
    s = _build(name)
    for a in (s.forecast, s.observed, s.mask):
        if a is not None:
            a.flags.writeable = False
    return s


@functools.lru_cache(maxsize=None)
def expected(name: str) -> Expected:
    s = scene(name)
    c = vo.contingency(s.forecast, s.observed, s.thresholds, s.mask)
    out = Expected(c.counts, c.valid, vo.sat(s.forecast, s.thresholds, s.observed, s.mask),
                   vo.sat(s.observed, s.thresholds, s.forecast, s.mask),
                   vo.fss_sums(s.forecast, s.observed, s.thresholds, s.scales, s.mask))
    for a in out:
        a.flags.writeable = False
    return out


# ---- the verifier's sequence ---------------------------------------------------------------------------------------------------
SEQ_SHAPE = (96, 128)
SEQ_FRAMES = 6
SEQ_MOTION = (3, -2)                    # (dy, dx) pixels per frame
SEQ_MARGIN = 40
SEQ_THRESHOLDS = (18.0, 35.0, 45.0, 70.0)      # the last one lies above every value: nothing reaches it
SEQ_SCALES = (1, 5, 33)
SEQ_LEADS = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def blob_sequence() -> np.ndarray:
    """float32 ``[6, 96, 128]``: a 5 dBZ background and a pattern of echoes of 20 .. 58 dBZ that moves ``SEQ_MOTION`` per
    frame and stays ``SEQ_MARGIN`` pixels from every border in all frames.  96 rows leave a band of 16 between the margins and
    the pattern travels 15, so it is one row high; it is 38 columns wide and travels 10 of the 48 between the margins."""
    h, w = SEQ_SHAPE
    rng = np.random.default_rng(29)
    pattern = np.where(rng.random(38) < 0.7, rng.uniform(20.0, 58.0, 38), 5.0).astype(np.float32)
    pattern[[0, -1]] = (50.0, 36.0)
    frames = np.full((SEQ_FRAMES, h, w), 5.0, dtype=np.float32)
    for k in range(SEQ_FRAMES):
        y, x = SEQ_MARGIN + k * SEQ_MOTION[0], w - SEQ_MARGIN - 38 + k * SEQ_MOTION[1]
        frames[k, y, x:x + 38] = pattern
    frames.flags.writeable = False
    return frames
