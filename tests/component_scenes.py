"""Scenes for the connected-component kernels: small planes, derived from the tile constants, at which the tile pass, the
seam pass and the numbering can still go wrong.  Every scene is ``Scene(name, planes [n, h, w] float32, lo, hi, mask, wrap)``;
``scenes(shape)`` builds them all for one plane shape, deterministically."""
import functools
import zlib
from typing import NamedTuple, Optional

import numpy as np

from radar_processor_amd import _native

TH, TW = _native.RG_CC_TILE_H, _native.RG_CC_TILE_W
# one pixel; one row / one column across two seams; exactly a tile; one pixel more both ways; several tiles with ragged edges
SHAPES = ((1, 1), (1, 2 * TW + 3), (2 * TH + 3, 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 5, 3 * TW + 7))
FIRST_RUN_SHAPES = ((1, 1), (TH, TW))
DENSITIES = (0.30, 0.41, 0.45, 0.593, 0.80)        # 0.41 / 0.593: the 8- / 4-connected percolation thresholds
LO = 35.0


class Scene(NamedTuple):
    name: str
    planes: np.ndarray
    lo: float
    hi: float
    mask: Optional[np.ndarray]
    wrap: bool


def _rng(name, shape):
    return np.random.default_rng(zlib.crc32(f"{name}:{shape}".encode()))


def _dress(name, pattern):
    """A boolean pattern [n, h, w] as reflectivity: foreground 35 .. 64.5 dBZ in 0.5 dB steps (ties are common), background a
    mix of NaN, values just below the threshold and -inf."""
    rng = _rng(name, pattern.shape)
    fg = (LO + 0.5 * rng.integers(0, 60, pattern.shape)).astype(np.float32)
    bg = rng.choice(np.array([np.nan, np.nan, LO - 0.5, 0.0, -np.inf], np.float32), pattern.shape)
    return np.where(pattern, fg, bg).astype(np.float32)


def serpentine(h, w):
    a = np.zeros((h, w), bool)
    a[0::2] = True
    for y in range(1, h, 2):
        a[y, w - 1 if (y // 2) % 2 == 0 else 0] = True
    return a


def spiral(h, w):
    """A one-pixel path that winds inwards, one pixel of background between its arms."""
    a = np.zeros((h, w), bool)
    y, x, dy, dx, turns = 0, 0, 0, 1, 0
    a[0, 0] = True
    while turns < 2:
        ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        free = 0 <= ny < h and 0 <= nx < w and not a[ny, nx] and not (0 <= fy < h and 0 <= fx < w and a[fy, fx])
        if free:
            y, x, turns = ny, nx, 0
            a[y, x] = True
        else:
            dy, dx, turns = dx, -dy, turns + 1
    return a


def comb(h, w):
    """Teeth on every other column that join only in the last row: the cell's first pixel lies far from the join."""
    a = np.zeros((h, w), bool)
    a[:, 0::2] = True
    a[h - 1] = True
    return a


def wrap_blob(h, w):
    """Three cells that touch row 0 and row h - 1: a column, a pair that meets only diagonally across the seam, and a pair
    two columns apart that never meets."""
    a = np.zeros((h, w), bool)
    a[:1, 0] = a[h - 1:, 0] = True
    for x0, gap in ((3, 1), (8, 2)):
        if x0 + gap < w:
            a[0, x0] = a[h - 1, x0 + gap] = True
    return a


@functools.lru_cache(maxsize=None)
def scenes(shape):
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    out = []

    def add(name, pattern, wrap=False):
        pattern = np.asarray(pattern, bool)
        pattern = pattern[None] if pattern.ndim == 2 else pattern
        out.append(Scene(name, _dress(name, pattern), LO, np.inf, None, wrap))

    out.append(Scene("all_nan", np.full((1, h, w), np.nan, np.float32), LO, np.inf, None, False))
    add("all_foreground", np.ones((h, w), bool))
    add("checkerboard", (yy + xx) % 2 == 0)
    add("diagonals", (xx - yy) % TH == 0)                      # through every tile corner
    add("antidiagonals", (xx + yy) % TH == TH - 1)             # ... and the other way
    add("serpentine", serpentine(h, w))
    add("spiral", spiral(h, w))
    add("comb", comb(h, w))
    for d in DENSITIES:
        add(f"random_{d}", _rng(f"random_{d}", shape).random((h, w)) < d)
    # values on a 0.5 dB lattice with pixels exactly at lo and at hi, NaN, +-inf, +-0, and a mask
    rng = _rng("lattice", shape)
    vals = (18.0 + 0.5 * rng.integers(0, 30, (1, h, w))).astype(np.float32)
    odd = rng.random((1, h, w))
    for k, special in enumerate((np.nan, np.inf, -np.inf, 0.0, -0.0, 20.0, 30.0)):
        vals[(odd >= 0.04 * k) & (odd < 0.04 * (k + 1))] = special
    out.append(Scene("lattice", vals, 20.0, 30.0, (rng.random((1, h, w)) < 0.1).astype(np.uint8), False))
    # signed zeros, +inf with an infinite upper bound: the total order of vmax / argmax, an infinite vsum
    zeros = rng.choice(np.array([0.0, -0.0, -0.0, 0.5, -0.5, -2.0, np.nan, np.inf], np.float32), (1, h, w))
    out.append(Scene("zeros", zeros.astype(np.float32), -1.0, np.inf, None, False))
    add("wrap_blob", wrap_blob(h, w), wrap=True)
    add("wrap_random_0.45", _rng("wrap_random", shape).random((h, w)) < 0.45, wrap=True)
    add("wrap_antidiagonals", (xx + yy) % max(h, 2) == 0, wrap=True)      # period h: each line goes on across the wrap seam
    add("wrap_serpentine", serpentine(h, w), wrap=True)
    # three planes, the middle one empty; the first ends and the third starts with foreground
    three = _rng("three", shape).random((3, h, w)) < 0.5
    three[1] = False
    three[0, h - 1, max(w - 3, 0):] = True
    three[2, 0, :3] = True
    add("three_planes", three)
    add("three_planes_wrap", three, wrap=True)
    return tuple(out)


def scene(shape, name):
    return next(s for s in scenes(shape) if s.name == name)


NON_WRAPPING = tuple(s.name for s in scenes((1, 1)) if not s.wrap)
WRAPPING = tuple(s.name for s in scenes((1, 1)) if s.wrap)
