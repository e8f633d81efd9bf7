"""Scenes for the accumulation tests (tests/test_accumulation_scenes.py, tests/test_gpu_accumulation.py): pairs of rate
planes, a motion field on one of three kinds of lattice, and the parameters of one ``rg_accumulate_advected_f32`` call.
Every scene and its restated result are computed once, shared, and read-only.

The kernel's workgroup covers a tile of 8 rows x 32 columns (``TILE``); the shapes are 1 x 1, 3 x 5 (less than one
wavefront), 37 x 53 (a width that is a multiple of neither 4 nor 64) and 19 x 70 (three tiles along either axis, the last
one cut).  Its threads keep the sums of at most four planes, so ``six_planes`` takes the second launch."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import accumulation_oracle as ao
import motion_oracle as mo

TILE = (8, 32)
FILL = -9.25


class Scene(NamedTuple):
    name: str
    prev: np.ndarray                    # float32 [P, h, w] mm/h
    next: np.ndarray
    motion: np.ndarray                  # float32 [ny, nx, 2]
    lattice: mo.Lattice
    hours: float
    n_steps: int
    substeps: int
    method: str
    min_steps: int
    fill: float
    holes: bool                         # the rates hold NaN (and +inf)


def rates(shape, planes, seed, holes):
    """float32 ``[planes, h, w]`` mm/h: a few smooth cells over dry ground (exact zeros); with ``holes`` also NaN -- a
    rectangle, single pixels -- and two +inf pixels per plane."""
    rng = np.random.default_rng(seed)
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((planes, h, w), dtype=np.float32)
    for p in range(planes):
        v = np.zeros(shape)
        for _ in range(5):
            cy, cx, sigma, peak = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(1.5, 6.0), rng.uniform(2.0, 90.0)
            v = np.maximum(v, peak * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * sigma * sigma)))
        v[v < 0.1] = 0.0
        if holes:
            y0, x0 = int(rng.integers(0, max(h - 3, 1))), int(rng.integers(0, max(w - 4, 1)))
            v[y0:y0 + max(h // 6, 1), x0:x0 + max(w // 6, 1)] = np.nan
            v[rng.random(shape) < 0.04] = np.nan
            for _ in range(2):
                v[int(rng.integers(0, h)), int(rng.integers(0, w))] = np.inf
        out[p] = v.astype(np.float32)
    return out


def dense_lattice(shape) -> mo.Lattice:
    return mo.Lattice(0.0, 0.0, 1.0, 1.0, shape[0], shape[1])


def one_node(vector, at=(0.0, 0.0)):
    return np.array([[vector]], dtype=np.float32), mo.Lattice(float(at[0]), float(at[1]), 1.0, 1.0, 1, 1)


def fractional(lat: mo.Lattice, seed, reach=6.0):
    return np.random.default_rng(seed).uniform(-reach, reach, (lat.ny, lat.nx, 2)).astype(np.float32)


def spreading(shape, gain):
    """A dense field that points away from the centre of the plane, ``gain`` pixels per pixel of distance: the later plane
    is sampled beyond every side, and with ``gain > 1`` the earlier one beyond the opposite side."""
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.stack([gain * (yy - (h - 1) / 2.0), gain * (xx - (w - 1) / 2.0)], axis=-1).astype(np.float32)


def _build(name: str) -> Scene:
    if name == "one_pixel":
        motion, lat = one_node((0.0, 0.0))
        return Scene(name, np.full((1, 1, 1), 4.5, np.float32), np.full((1, 1, 1), 1.25, np.float32), motion, lat, 0.25, 1, 1,
                     "nearest", 1, FILL, False)
    if name == "one_pixel_bilinear":                      # a fractional vector: the taps' weights fall below 0.5 on the way
        motion, lat = one_node((0.75, -0.5), at=(3.0, -2.0))
        return Scene(name, np.full((1, 1, 1), 4.5, np.float32), np.full((1, 1, 1), 1.25, np.float32), motion, lat, 0.25, 7, 3,
                     "bilinear", 1, FILL, False)
    if name == "tiny_uniform":
        motion, lat = one_node((1.0, -2.0))
        return Scene(name, rates((3, 5), 3, 1, False), rates((3, 5), 3, 2, False), motion, lat, 1.0 / 12.0, 3, 1, "bilinear", 2,
                     FILL, False)
    if name == "tiny_holes":
        motion, lat = one_node((-1.0, 1.0))
        return Scene(name, rates((3, 5), 1, 3, True), rates((3, 5), 1, 4, True), motion, lat, 0.1, 7, 1, "nearest", 4, np.nan, True)
    if name in ("dense_bilinear", "dense_nearest"):
        shape = (37, 53)
        lat = dense_lattice(shape)
        bil = name == "dense_bilinear"
        return Scene(name, rates(shape, 3 if bil else 1, 5, True), rates(shape, 3 if bil else 1, 6, True), fractional(lat, 7), lat,
                     1.0 / 6.0, 7, 3 if bil else 1, "bilinear" if bil else "nearest", 4 if bil else 7, np.nan if bil else FILL, True)
    if name in ("block_64", "block_sub3"):
        shape = (37, 53)
        lat = mo.block_lattice(shape, 8, 4)
        first = name == "block_64"
        return Scene(name, rates(shape, 1 if first else 3, 8, True), rates(shape, 1 if first else 3, 9, True), fractional(lat, 10),
                     lat, 0.125, 64 if first else 3, 1 if first else 3, "bilinear" if first else "nearest", 32 if first else 1, FILL,
                     True)
    if name in ("outside_bilinear", "outside_nearest"):
        shape = (19, 70)
        bil = name == "outside_bilinear"
        return Scene(name, rates(shape, 1 if bil else 3, 11, True), rates(shape, 1 if bil else 3, 12, True), spreading(shape, 2.6),
                     dense_lattice(shape), 0.25, 7 if bil else 64, 1 if bil else 3, "bilinear" if bil else "nearest",
                     6 if bil else 60, FILL, True)
    if name == "uniform_integer":
        motion, lat = one_node((3.0, -5.0), at=(9.0, 30.0))
        return Scene(name, rates((19, 70), 1, 13, True), rates((19, 70), 1, 14, True), motion, lat, 5.0 / 60.0, 7, 1, "nearest", 7,
                     np.nan, True)
    if name == "six_planes":
        shape = (19, 70)
        lat = mo.block_lattice(shape, 8, 4)
        return Scene(name, rates(shape, 6, 15, True), rates(shape, 6, 16, True), fractional(lat, 17, 4.0), lat, 0.2, 3, 1, "bilinear", 2,
                     np.nan, True)
    if name == "zero_motion":
        motion, lat = one_node((0.0, 0.0))
        return Scene(name, rates((19, 70), 3, 18, False), rates((19, 70), 3, 19, False), motion, lat, 0.5, 7, 1, "bilinear", 7, FILL,
                     False)
    if name == "steady":                                  # prev == next, one step, no motion: hours * rate
        motion, lat = one_node((0.0, 0.0))
        r = rates((37, 53), 1, 20, False)
        return Scene(name, r, r, motion, lat, 0.75, 1, 1, "nearest", 1, FILL, False)
    raise KeyError(name)


SCENES = ("one_pixel", "one_pixel_bilinear", "tiny_uniform", "tiny_holes", "dense_bilinear", "dense_nearest", "block_64",
          "block_sub3", "outside_bilinear", "outside_nearest", "uniform_integer", "six_planes", "zero_motion", "steady")
COMPOSED = ("dense_bilinear", "outside_nearest")          # also held against the composition of rg_advect_f32


@functools.lru_cache(maxsize=None)
def scene(name: str) -> Scene:
    s = _build(name)
    for a in (s.prev, s.next, s.motion):
        a.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def expected(name: str) -> ao.Accumulation:
    """The restated result of a scene -- computed once, shared, never modified."""
    s = scene(name)
    want = ao.accumulate(s.prev, s.next, s.motion, s.lattice, s.hours, s.n_steps, s.substeps, s.method, s.min_steps, s.fill)
    want.out.setflags(write=False)
    want.steps.setflags(write=False)
    return want


def is_fill(out, fill):
    """Where ``out`` holds the bits of ``fill``."""
    return np.ascontiguousarray(out, dtype=np.float32).view(np.uint32) == np.float32(fill).reshape(1).view(np.uint32)[0]


# ---- the moving pixel ---------------------------------------------------------------------------------------------------------
MOVING_RATE, MOVING_HOURS, MOVING_SHAPE = 12.0, 0.25, (5, 20)


def moving_pixel():
    """One pixel of 12 mm/h at column 5 of the earlier plane and column 13 of the later one, a quarter of an hour apart, over
    dry ground: ``(prev, next, motion, lattice)`` with the true motion (0, 8)."""
    prev, nxt = np.zeros((1,) + MOVING_SHAPE, np.float32), np.zeros((1,) + MOVING_SHAPE, np.float32)
    prev[0, 2, 5] = nxt[0, 2, 13] = MOVING_RATE
    motion, lat = one_node((0.0, 8.0))
    return prev, nxt, motion, lat


# ---- the accumulator's frames -------------------------------------------------------------------------------------------------
FRAME_SHAPE, FRAME_MOTION, FRAME_SECONDS, FRAME_START = (48, 64), (3.0, -2.0), 300.0, (18.0, 40.0)
FRAME_ESTIMATE = dict(block=16, stride=8, search=6)


def frames(count=4):
    """float32 ``[count, 48, 64]`` dBZ: one compact cell of 50 dBZ over dry ground (0 dBZ) that moves (3, -2) pixels per
    frame; the coordinates are displaced, not the values, so every frame holds the same float32 numbers."""
    h, w = FRAME_SHAPE
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((count, h, w), dtype=np.float32)
    for t in range(count):
        cy, cx = FRAME_START[0] + t * FRAME_MOTION[0], FRAME_START[1] + t * FRAME_MOTION[1]
        out[t] = (50.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * 1.2 * 1.2))).astype(np.float32)
    out.setflags(write=False)
    return out


def centroid_path(first, last):
    """The pixels ``(y, x)`` nearest to the cell's centre from frame ``first`` to frame ``last``, in sixths of a frame."""
    out = []
    for k in range(6 * (last - first) + 1):
        t = first + k / 6.0
        p = (int(np.floor(FRAME_START[0] + t * FRAME_MOTION[0] + 0.5)), int(np.floor(FRAME_START[1] + t * FRAME_MOTION[1] + 0.5)))
        if p not in out:
            out.append(p)
    return out
