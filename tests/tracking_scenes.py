"""Scenes for the cell-overlap kernels and the tracker: pairs of small label stacks at which the run detection, the hash table
and the row arithmetic can still go wrong, and a four-frame sequence of moving blobs.  Label planes come from
``components_oracle.label``; nothing is above 69 x 199.  Every overlap scene is ``Scene(name, labels_prev, ptr_prev,
labels_next, ptr_next)`` with int32 ``[n, h, w]`` labels and int32 ``[n + 1]`` running cell counts."""
import functools
import zlib
from typing import NamedTuple

import numpy as np

import components_oracle as co

LO = 35.0
BIG = (69, 199)
THRESHOLDS = (0.45, 0.55, 0.65)          # of the smoothed noise below: many small cells, fewer, a handful


class Scene(NamedTuple):
    name: str
    labels_prev: np.ndarray
    ptr_prev: np.ndarray
    labels_next: np.ndarray
    ptr_next: np.ndarray


def _label(pattern, connectivity=8):
    pattern = np.asarray(pattern, bool)
    pattern = pattern[None] if pattern.ndim == 2 else pattern
    return co.label(np.where(pattern, np.float32(40.0), np.float32(np.nan)), LO, connectivity=connectivity)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def smooth_noise(name, shape):
    """Uniform noise averaged three times over 5 x 5 neighbourhoods (wrapping): blobs of a few pixels to a few dozen."""
    a = _rng(name).random(shape)
    for _ in range(3):
        a = sum(np.roll(a, (dy, dx), (0, 1)) for dy in range(-2, 3) for dx in range(-2, 3)) / 25.0
    return (a - a.min()) / (a.max() - a.min())


def shifted(pattern, dy, dx):
    """``pattern`` moved by ``(dy, dx)``, background moving in."""
    h, w = pattern.shape
    out = np.zeros_like(pattern)
    out[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)] = pattern[max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)]
    return out


def checkerboard(h=32, w=64):
    yy, xx = np.mgrid[0:h, 0:w]
    return (yy + xx) % 2 == 0


@functools.lru_cache(maxsize=None)
def scenes():
    out = []

    def add(name, prev, nxt, conn_prev=8, conn_next=8):
        out.append(Scene(name, *_label(prev, conn_prev), *_label(nxt, conn_next)))

    add("1x1", np.ones((1, 1), bool), np.ones((1, 1), bool))
    row = np.ones((1, 130), bool)
    cut = row.copy()
    cut[0, 100] = False                                                  # runs 0 .. 99 and 101 .. 129: over both seams
    add("1x130", row, cut)
    col = np.ones((67, 1), bool)
    gaps = col.copy()
    gaps[20::20] = False
    add("67x1", gaps, col)
    for h, w in ((33, 65), BIG):
        add(f"all_{h}x{w}", np.ones((h, w), bool), np.ones((h, w), bool))
    add("checker_both", checkerboard(), checkerboard(), 4, 4)
    add("checker_vs_all", checkerboard(), np.ones((32, 64), bool), 4, 8)
    noise = smooth_noise("blobs", BIG)
    for t in THRESHOLDS:
        add(f"blobs_{t}", noise >= t, shifted(noise >= t, 2, -3))
    left = np.zeros(BIG, bool)
    left[:, :90] = noise[:, :90] >= 0.5
    right = np.zeros(BIG, bool)
    right[:, 110:] = noise[:, 110:] >= 0.5
    add("disjoint", left, right)
    add("empty_next", noise >= 0.5, np.zeros(BIG, bool))
    # labels above the plane's cell count and below zero, planted by hand: they take no part
    s = Scene("planted", *_label(noise >= 0.55), *_label(shifted(noise >= 0.55, 1, 2)))
    lp, ln = s.labels_prev.copy(), s.labels_next.copy()
    rng = _rng("planted")
    for labels, ptr in ((lp, s.ptr_prev), (ln, s.ptr_next)):
        at = rng.integers(0, labels.size, 300)
        labels.ravel()[at] = rng.choice(np.array([int(ptr[-1]) + 1, int(ptr[-1]) + 7, 2 ** 31 - 1, -3], np.int32), 300)
    out.append(s._replace(labels_prev=lp, labels_next=ln))
    # a stack of three planes with different cell counts, paired as L[:-1] / L[1:]; the next frames keep the rows of the stack
    stack = np.stack([noise >= 0.45, shifted(noise >= 0.6, 2, -3), shifted(noise >= 0.5, 4, -6)])
    labels, ptr = _label(stack)
    out.append(Scene("stack", labels[:-1], ptr[:-1].copy(), labels[1:], ptr[1:].copy()))
    for s in out:
        for a in s[1:]:
            a.setflags(write=False)
    return tuple(out)


def scene(name):
    return next(s for s in scenes() if s.name == name)


NAMES = tuple(s.name for s in scenes())


# ---- the tracker's sequence --------------------------------------------------------------------------------------------------
FRAMES = 4
BACKGROUND = 10.0
SHIFT = (2, -3)                          # pixels per frame: every blob overlaps itself from frame to frame
FAST_SHIFT = (1, -16)                    # further than any blob is wide: nothing overlaps without advection


def _disc(plane, cy, cx, r):
    """A paraboloid of 36 .. 50 dBZ over the pixels within ``r`` of the centre: at or above ``LO`` exactly there."""
    yy, xx = np.mgrid[0:plane.shape[0], 0:plane.shape[1]]
    d2 = ((yy - cy) ** 2 + (xx - cx) ** 2) / float(r * r)
    np.maximum(plane, np.where(d2 <= 1.0, 36.0 + 14.0 * (1.0 - d2), BACKGROUND), out=plane)


@functools.lru_cache(maxsize=None)
def tracker_frames(shift=SHIFT):
    """Four float32 planes ``69 x 199``, everything translating by ``shift`` per frame:

    A   a disc that only moves;
    B   two discs of radius 5 and 4 that are one cell in frames 0 and 1 and two cells from frame 2 on (a split);
    C, D   discs of radius 5 and 3, two cells until frame 2 and one cell in frame 3 (a merge);
    E   a disc that appears in frame 1 (a birth);
    F   a small disc at the western rim that has left the plane by frame 3 under ``SHIFT`` (a death)."""
    dy, dx = shift
    frames = []
    for t in range(FRAMES):
        plane = np.full(BIG, BACKGROUND, dtype=np.float64)
        oy, ox = t * dy, t * dx
        _disc(plane, 15 + oy, 150 + ox, 6)                                       # A
        _disc(plane, 45 + oy, 100 + ox, 5)                                       # B, the larger part
        _disc(plane, 45 + oy, 100 + ox + (6 if t < 2 else 13), 4)               # B, the smaller part
        _disc(plane, 20 + oy, 60 + ox, 5)                                        # C
        _disc(plane, 20 + oy, 60 + ox + (12 if t < 3 else 6), 3)                # D
        if t >= 1:
            _disc(plane, 52 + oy, 185 + ox, 5)                                   # E
        _disc(plane, 30 + oy, 5 + ox, 3)                                         # F
        plane = plane.astype(np.float32)
        plane.setflags(write=False)
        frames.append(plane)
    return tuple(frames)
