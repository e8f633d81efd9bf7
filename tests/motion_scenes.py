"""Scenes for the echo-motion tests (tests/test_motion_oracle.py, tests/test_gpu_motion.py): synthetic plane pairs whose true
motion is known, the degenerate inputs of the contract, and the extremes of the parameter ranges.  Every scene, its levels
and its restated match are computed once, shared, and read-only.

The echo field is a maximum of Gaussians evaluated ANALYTICALLY at displaced coordinates, so a displaced frame is exact --
no resampling -- and for an integer displacement it holds the same float32 values as the first frame, moved.
``B=16, S=8, R=6`` unless a scene says otherwise."""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional, Tuple

import numpy as np

import motion_oracle as mo

B, S, R = 16, 8, 6
LO, HI = 0.0, 63.5
ECHO_FLOOR = 5.0                        # dBZ below which the analytic field is NaN


class Scene(NamedTuple):
    name: str
    prev: np.ndarray                    # float32 or uint8 levels, [h, w] or [n, h, w]
    next: np.ndarray
    B: int = B
    S: int = S
    R: int = R
    min_echo: Optional[int] = None      # None: B * B // 8
    mask_prev: Optional[np.ndarray] = None
    mask_next: Optional[np.ndarray] = None
    truth: Optional[Tuple[float, float]] = None     # (dy, dx) of the whole field


def blobs(shape, seed, count):
    """``count`` Gaussians ``(cy, cx, sigma, peak dBZ)`` scattered over a plane of ``shape`` and a margin around it."""
    rng = np.random.default_rng(seed)
    h, w = shape
    return np.stack([rng.uniform(-0.15 * h, 1.15 * h, count), rng.uniform(-0.15 * w, 1.15 * w, count),
                     rng.uniform(2.5, 6.0, count), rng.uniform(25.0, 60.0, count)], axis=1)


def field(shape, table, offset=(0.0, 0.0)) -> np.ndarray:
    """The echo of ``table`` displaced by ``offset`` = (dy, dx): float32 ``[h, w]``, NaN below :data:`ECHO_FLOOR`.  The
    displacement is subtracted from the pixel coordinates FIRST, so an integer offset moves the values bit for bit."""
    h, w = shape
    y = np.arange(h, dtype=np.float64)[:, None] - float(offset[0])
    x = np.arange(w, dtype=np.float64)[None, :] - float(offset[1])
    v = np.zeros((h, w))
    for cy, cx, sigma, peak in table:
        v = np.maximum(v, peak * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2.0 * sigma * sigma)))
    out = v.astype(np.float32)
    out[v < ECHO_FLOOR] = np.nan
    return out


def translated(shape, seed, count, motion, times=(0.0, 1.0)) -> np.ndarray:
    """Frames ``[len(times), h, w]`` of one field moving by ``motion`` per unit of time."""
    table = blobs(shape, seed, count)
    return np.stack([field(shape, table, (t * motion[0], t * motion[1])) for t in times])


NOWCAST_SHAPE, NOWCAST_SEED, NOWCAST_BLOBS, NOWCAST_MARGIN = (96, 112), 21, 60, 20
NOWCAST_MOTIONS = {"integer": (3.0, -5.0), "subpixel": (1.5, -2.25)}


def nowcast_frames(kind: str, times) -> np.ndarray:
    """The 96 x 112 translated field of the nowcast tests at ``times`` (frame 0 and 1 are the pair, 1 + lead the truth)."""
    return translated(NOWCAST_SHAPE, NOWCAST_SEED, NOWCAST_BLOBS, NOWCAST_MOTIONS[kind], times)


def _stripes(shape, shift):
    """Vertical stripes of period 4, levels 10, 10, 40, 40, moved ``shift`` columns to the right."""
    h, w = shape
    return np.broadcast_to(np.array([10, 10, 40, 40], dtype=np.uint8)[(np.arange(w) - shift) % 4], (h, w)).copy()


def _min_echo_levels():
    """16 x 32 levels, two blocks at stride 16: the left one holds min_echo - 1 = 31 echo pixels, the right one 32."""
    q = np.zeros((16, 32), dtype=np.uint8)
    ramp = (np.arange(32) * 7 % 200 + 20).astype(np.uint8)
    q[3, 0:16], q[4, 0:15] = ramp[:16], ramp[16:31]
    q[3, 16:32], q[4, 16:32] = ramp[:16], ramp[16:]
    return q


def _build(name: str) -> Scene:
    if name == "shift":
        f = translated((61, 83), 7, 40, (3.0, -5.0))
        return Scene(name, f[0], f[1], truth=(3.0, -5.0))
    if name == "subpixel":
        f = translated((61, 83), 7, 40, (1.5, -2.25))
        return Scene(name, f[0], f[1], truth=(1.5, -2.25))
    if name == "rim":      # w odd, neither side a multiple of the stride, echo on all four edges.  R = 8: with 6 the last
        # column of blocks (x0 = 48, 7 free columns to its right) would keep every candidate -- no clipping in the east
        table = np.concatenate([blobs((45, 71), 11, 30), [[0.0, 20.0, 5.0, 50.0], [44.0, 50.0, 5.0, 55.0],
                                                           [22.0, 0.0, 5.0, 45.0], [25.0, 70.0, 5.0, 52.0]]])
        return Scene(name, field((45, 71), table), field((45, 71), table, (-2.0, 4.0)), R=8, truth=(-2.0, 4.0))
    if name == "ties":
        return Scene(name, _stripes((40, 56), 0), _stripes((40, 56), 2))
    if name == "degenerate_constant":
        plane = np.full((33, 41), 30.0, dtype=np.float32)
        return Scene(name, plane, plane.copy())
    if name == "degenerate_all_nan":
        plane = np.full((33, 41), np.nan, dtype=np.float32)
        return Scene(name, plane, plane.copy())
    if name == "degenerate_min_echo":
        q = _min_echo_levels()
        return Scene(name, q, q.copy(), S=16, min_echo=32)
    if name == "degenerate_levels":                       # lo, just below lo, hi, above hi and both infinities in a live field
        f = translated((35, 43), 5, 24, (1.0, 1.0))
        for k, v in enumerate((LO, np.nextafter(np.float32(LO), np.float32(-1.0)), HI, np.nextafter(np.float32(HI), np.float32(99.0)),
                               80.0, np.inf, -np.inf, -3.0, HI - 0.125, LO + 0.25, 0.2499)):
            f[0, 9 + k, 12 + k], f[1, 10 + k, 13 + k] = v, v
        return Scene(name, f[0], f[1], truth=(1.0, 1.0))
    if name == "degenerate_masked":
        f = translated((61, 83), 7, 40, (3.0, -5.0))
        mp, mn = np.zeros((61, 83), dtype=np.uint8), np.zeros((61, 83), dtype=np.uint8)
        mp[14:34, 30:50], mn[5:16, 60:83] = 1, 7          # prev: block (2, 4) = [16:32, 32:48] is masked whole
        return Scene(name, f[0], f[1], mask_prev=mp, mask_next=mn, truth=(3.0, -5.0))
    if name == "extremes_64_32":
        f = translated((130, 140), 13, 90, (7.0, -11.0))
        return Scene(name, f[0], f[1], B=64, R=32, truth=(7.0, -11.0))
    if name in ("extremes_4_0", "extremes_8_1"):
        table = [[4.0, 6.0, 3.0, 55.0], [1.0, 1.0, 1.5, 40.0], [7.0, 11.0, 2.0, 48.0]]
        f = np.stack([field((9, 13), table), field((9, 13), table, (0.0, 1.0))])
        return Scene(name, f[0], f[1], B=4, R=0) if name == "extremes_4_0" else Scene(name, f[0], f[1], B=8, R=1)
    if name == "stack":                                   # three pairs in one call: q[:-1] and q[1:] of four planes
        table = blobs((61, 83), 7, 40)
        f = np.stack([field((61, 83), table, off) for off in ((0.0, 0.0), (3.0, -5.0), (4.5, -7.25), (4.5, -2.25))])
        return Scene(name, f[:-1], f[1:])
    raise KeyError(name)


DEGENERATE = ("degenerate_constant", "degenerate_all_nan", "degenerate_min_echo", "degenerate_levels", "degenerate_masked")
EXTREMES = ("extremes_64_32", "extremes_4_0", "extremes_8_1")
SCENES = ("shift", "subpixel", "rim", "ties") + DEGENERATE + EXTREMES + ("stack",)


@functools.lru_cache(maxsize=None)
def scene(name: str) -> Scene:
    s = _build(name)
    for a in (s.prev, s.next, s.mask_prev, s.mask_next):
        if a is not None:
            a.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def levels(name: str, masked: bool = True):
    """``(prev, next)`` uint8 levels of a scene by the restatement (a scene of levels is returned as it is)."""
    s = scene(name)
    if s.prev.dtype == np.uint8:
        return s.prev, s.next
    out = (mo.quantize(s.prev, LO, HI, s.mask_prev if masked else None), mo.quantize(s.next, LO, HI, s.mask_next if masked else None))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def match(name: str) -> mo.Match:
    """The restated block match of a scene -- computed once, shared, never modified."""
    s = scene(name)
    m = mo.block_match(*levels(name), s.B, s.S, s.R, s.min_echo)
    for a in m:
        a.setflags(write=False)
    return m


def inner(a):
    """The blocks not on the lattice's outer ring: ``a[..., 1:-1, 1:-1]`` of a ``[n, nby, nbx]`` array."""
    return a[:, 1:-1, 1:-1]
