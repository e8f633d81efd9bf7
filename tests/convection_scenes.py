"""Scenes for the convection tests (tests/test_convection_scenes.py, tests/test_gpu_convection.py): dBZ planes, an optional
mask, the background footprint, one footprint per radius class, the class edges and the scalars.  Every scene and its
restated result are computed once, shared, and read-only.

The kernels walk a row in trips of 64 pixels (the tables) or give 64 pixels of four rows to a workgroup (the footprint sums),
so the widths are 100 (two trips, no multiple of 4 or 64), 257 and 64 (a trip seam with one pixel beyond it, exactly one
trip), 150 under a 127-pixel footprint (every footprint cut on three sides), 1 and 300."""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional, Tuple

import numpy as np

import convection_oracle as co

DY, DX = 500.0, 400.0                                  # metres per pixel of the main scenes
BACKGROUND_RADIUS = 11000.0
EDGES = (25.0, 30.0, 35.0, 40.0)                       # the "medium" relation
RADII = (1000.0, 2000.0, 3000.0, 4000.0, 5000.0)
MAIN = ("main_35", "main_39")                          # seeds without a fragile decision and with every class (see the tests)
SCENES = MAIN + ("stack", "seam_257", "seam_64", "tall_disk", "big_sums", "one_pixel", "one_row", "one_column", "non_monotone",
                 "box")
FRAGILE_DB = 1e-3


class Scene(NamedTuple):
    name: str
    dbz: np.ndarray                        # float32 [n, h, w]
    mask: Optional[np.ndarray]             # uint8 [n, h, w] or None
    hw: Tuple[int, ...]                    # the background footprint
    footprints: Tuple[Tuple[int, ...], ...]      # one per radius class
    edges: Tuple[float, ...]
    min_dbz: float = 5.0
    intense: float = 40.0
    peak: Tuple[float, float] = co.STEINER


class Expected(NamedTuple):
    q: np.ndarray                          # int64 [n, h, w]
    echo: np.ndarray                       # bool
    S: np.ndarray                          # int64
    N: np.ndarray                          # int32
    bkg: np.ndarray                        # float32
    centres: np.ndarray                    # uint8
    classes: np.ndarray                    # uint8


def footprint(radius_m: float, dy: float = DY, dx: float = DX) -> Tuple[int, ...]:
    """The disk footprint by the brute-force distance test (``radar_processor_amd.disk_footprint`` is tested against it)."""
    return co.disk_footprint_brute(radius_m, dy, dx)


def field(seed: int, shape, nan_share: float = 0.03, mask_share: float = 0.02):
    """``(dbz float32 [h, w], mask uint8 [h, w])``: a smooth field of 0 dBZ or more, six Gaussian cells, N(0, 1.5) noise,
    ``nan_share`` NaN pixels, a NaN block on the west rim and ``mask_share`` masked pixels."""
    h, w = shape
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    f = 14.0 + 8.0 * np.sin(x / 23.0 + seed) * np.cos(y / 17.0) + 4.0 * y / h
    for _ in range(6):
        cy, cx = rng.uniform(4, max(h - 4, 5)), rng.uniform(4, max(w - 4, 5))
        amp, sig = rng.uniform(12, 42), rng.uniform(1.5, 9.0)
        f += amp * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * sig * sig))
    f += rng.normal(0, 1.5, shape)
    f = np.maximum(f, 0.0).astype(np.float32)
    f[rng.random(shape) < nan_share] = np.nan
    f[(5 * h) // 18:(5 * h) // 8, 0:min(6, w // 2)] = np.nan
    mask = (rng.random(shape) < mask_share).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)
    return f, mask


def _disks(dy=DY, dx=DX):
    return footprint(BACKGROUND_RADIUS, dy, dx), tuple(footprint(r, dy, dx) for r in RADII)


def _build(name: str) -> Scene:
    hw, fps = _disks()
    if name.startswith("main_"):                          # 72 x 100, ry = 22, hw <= 27
        f, m = field(int(name[5:]), (72, 100))
        return Scene(name, f[None], m[None], hw, fps, EDGES)
    if name == "stack":                                   # the middle plane has no echo at all
        a, ma = field(3, (40, 90))
        c, mc = field(4, (40, 90))
        quiet = np.full((40, 90), 4.75, np.float32)
        quiet[::7, ::5] = np.nan
        return Scene(name, np.stack([a, quiet, c]), np.stack([ma, np.zeros_like(ma), mc]), hw, fps, EDGES)
    if name == "seam_257":
        f, m = field(5, (70, 257))
        return Scene(name, f[None], m[None], hw, fps, EDGES)
    if name == "seam_64":
        f, _ = field(6, (33, 64))
        return Scene(name, f[None], None, hw, fps, EDGES)
    if name == "tall_disk":                               # the plane is shorter than the disk: ry = 127 on 40 rows
        f, m = field(7, (40, 150))
        big = footprint(12750.0, 100.0, 100.0)
        assert len(big) == 128 and max(big) == 127
        return Scene(name, f[None], m[None], big, (fps[0], fps[2], big), (34.49, 34.6))     # the background hardly varies
    if name == "big_sums":                                # S ~ 3.3e17: beyond 2^53, float64's exact integers
        big = footprint(12750.0, 100.0, 100.0)
        return Scene(name, np.full((1, 260, 260), 85.0, np.float32), None, big, (fps[1],), ())
    if name == "one_pixel":
        return Scene(name, np.full((1, 1, 1), 41.0, np.float32), None, hw, fps, EDGES)
    if name == "one_row":
        f, m = field(8, (1, 300))
        return Scene(name, f[None], m[None], hw, fps, EDGES)
    if name == "one_column":
        f, m = field(9, (300, 1))
        return Scene(name, f[None], m[None], hw, fps, EDGES)
    if name == "non_monotone":                            # half-widths that grow and shrink with the row distance
        f, m = field(10, (50, 90))
        return Scene(name, f[None], m[None], (3, 9, 0, 12, 1, 0, 7), ((0, 2, 0, 3), (1,), (2, 0, 0, 0, 5), (0,), (4, 4, 1)), EDGES)
    if name == "box":                                     # 11 x 21 and smaller boxes
        f, m = field(11, (50, 90))
        return Scene(name, f[None], m[None], (10,) * 6, ((1, 1), (2,) * 3, (3,) * 2, (4,) * 5, (5,) * 6), EDGES)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def scene(name: str) -> Scene:
    s = _build(name)
    for a in (s.dbz, s.mask):
        if a is not None:
            a.flags.writeable = False
    return s


@functools.lru_cache(maxsize=None)
def expected(name: str) -> Expected:
    """The prefix oracle's result with NumPy's own q."""
    s = scene(name)
    q, e = co.quantize(s.dbz, s.mask, s.min_dbz), co.echo(s.dbz, s.mask, s.min_dbz)
    S, N, bkg = co.background(s.dbz, s.hw, s.mask, s.min_dbz, q)
    c = co.centres(s.dbz, bkg, s.edges, s.mask, s.min_dbz, s.intense, s.peak)
    out = Expected(q, e, S, N, bkg, c, co.area(c, s.dbz, s.footprints, s.mask, s.min_dbz))
    for a in out:
        a.flags.writeable = False
    return out


def margins(name: str):
    """``(intensity, peakedness, edge)``: the smallest distance in dB of any echo pixel's ``v`` from ``intense``, of any echo
    pixel's ``v - b`` from ``delta(b)``, and of any centre's ``b`` from an edge.  A decision closer than ``FRAGILE_DB`` could
    flip under one float32 step of the background or a one-unit tie of q."""
    s, want = scene(name), expected(name)
    v, b = s.dbz.astype(np.float64)[want.echo], want.bkg.astype(np.float64)[want.echo]
    at_centres = want.bkg.astype(np.float64)[want.centres > 0]
    edge = min((float(np.abs(at_centres - e).min()) for e in s.edges), default=np.inf) if at_centres.size else np.inf
    return float(np.abs(v - s.intense).min()), float(np.abs((v - b) - co.peak_delta(b, s.peak)).min()), edge


# ---- known answers -------------------------------------------------------------------------------------------------------------
def uniform(value: float, shape=(30, 40)) -> np.ndarray:
    out = np.full((1,) + tuple(shape), value, np.float32)
    out.flags.writeable = False
    return out


def spike(shape=(31, 41), base: float = 20.0, peak: float = 35.0):
    """``(planes, (y, x))``: ``base`` everywhere and one pixel of ``peak`` in the middle."""
    out = np.full((1,) + tuple(shape), base, np.float32)
    y, x = shape[0] // 2, shape[1] // 2
    out[0, y, x] = peak
    out.flags.writeable = False
    return out, (y, x)


def footprint_mask(hw, shape, centre) -> np.ndarray:
    """bool ``[h, w]``: the pixels of footprint ``hw`` around ``centre``."""
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    dy, dx = np.abs(y - centre[0]), np.abs(x - centre[1])
    half = np.asarray(tuple(hw) + (-1,))[np.minimum(dy, len(hw))]
    return dx <= half
