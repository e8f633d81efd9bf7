"""Scenes for the probabilistic nowcasts (csrc/rg_ensemble.hip), each built to reach one thing; tests/test_ensemble_scenes.py
asserts on the CPU, through the oracle alone, that it does.

``rim``          37 x 53 (neither a multiple of 4 or 64; seven full workgroups and a remainder), 5 members, shifts up to +-60
                 pixels: pixels with no member, with 1 .. 4 and with all 5 occur; run at ``min_members`` 1 and 5;
``caps``         20 x 70, 64 members, 8 thresholds, 16 leads, 16 substeps: pixels where all 64 members exceed all 8 thresholds,
                 so every 8-bit field of the packed counts holds 64;
``ties``         values equal to a threshold, +-inf, -0.0 against the threshold 0.0, NaN holes; nearest, so values are copied;
``lattice``      70 x 129 under a 3 x 4 node lattice, 3 substeps, bilinear, fractional shifts: weight sums on both sides of 0.5
                 next to the NaN holes;
``slivers``      1 x 1, 1 x 200 and 200 x 1;
``trips``        one plane of more than ``kHistMaxStrips * kBlock`` pixels through the histogram: its workgroups walk a second
                 trip of the grid-stride loop, some of them only one (the cap is READ from the kernel source);
``many_planes``  4099 planes of 2 x 3 through the histogram;
``planted``      counts above M, incomplete (and overfull) ``members``, masked and NaN observations planted in the histogram's
                 inputs.

Everything is deterministic, computed once, read-only, and importable without a GPU."""
import functools
import os
import re
from typing import NamedTuple

import numpy as np

import ensemble_oracle as eo
import motion_oracle as mo

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "radar_processor_amd", "csrc")


def _constant(source, name):
    """``<name> = <integer>`` inside a ``constexpr int`` statement of a kernel source, or None when it is not there."""
    with open(os.path.join(_CSRC, source)) as f:
        found = re.search(r"^\s*constexpr\s+int\s+[^;]*\b%s\s*=\s*(\d+)\s*[,;]" % name, f.read(), flags=re.M)
    return int(found.group(1)) if found else None


BLOCK = _constant("rg_common.hpp", "kBlock")
HIST_MAX_STRIPS = _constant("rg_ensemble.hip", "kHistMaxStrips")


class Scene(NamedTuple):
    src: np.ndarray             # float32 [h, w]
    motion: np.ndarray          # float32 [ny, nx, 2]
    lattice: mo.Lattice
    leads: tuple
    shifts: np.ndarray          # float64 [L, M, 2]
    thresholds: np.ndarray      # float32 [T]
    substeps: int
    method: str
    min_members: int

    @property
    def n_members(self):
        return self.shifts.shape[1]


class HistScene(NamedTuple):
    counts: np.ndarray          # uint8 [n, T, h, w]
    members: np.ndarray         # uint8 [n, h, w]
    obs: np.ndarray             # float32 [n, h, w]
    mask: object                # uint8 [n, h, w] or None
    n_members: int
    thresholds: np.ndarray


def _frozen(scene):
    for a in scene:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return scene


def _dense(h, w):
    return mo.Lattice(0.0, 0.0, 1.0, 1.0, h, w)


def _field(rng, h, w, lo=-5.0, hi=62.0, holes=0.06):
    """A smooth-ish float32 plane with NaN holes: a few blobs over a noisy floor."""
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    v = rng.uniform(lo, lo + 15.0, size=(h, w))
    for _ in range(4):
        cy, cx, s = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(2.0, max(h, w) / 3.0 + 2.0)
        v += (hi - lo) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * s * s))
    v = np.minimum(v, hi).astype(np.float32)
    v[rng.random((h, w)) < holes] = np.nan
    return v


def _swirl(h, w, ny, nx, amp):
    """float32 [ny, nx, 2]: a motion field that varies over the lattice."""
    jj, ii = np.meshgrid(np.linspace(-1.0, 1.0, ny) if ny > 1 else np.zeros(1), np.linspace(-1.0, 1.0, nx) if nx > 1 else np.zeros(1),
                         indexing="ij")
    return np.stack([amp * (0.6 + 0.4 * ii - 0.3 * jj), amp * (-0.8 + 0.5 * jj + 0.2 * ii)], axis=-1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def rim(min_members=1) -> Scene:
    rng = np.random.default_rng(101)
    h, w = 37, 53
    shifts = np.zeros((3, 5, 2))
    shifts[0] = rng.uniform(-1.5, 1.5, size=(5, 2))                          # all five inside nearly everywhere
    shifts[1] = [[0.0, 0.0], [11.25, -17.5], [-14.0, 20.5], [60.0, 3.0], [-2.5, -60.0]]      # two members never inside
    shifts[2] = [[60.0, 0.0], [-60.0, 1.0], [0.5, 60.0], [-1.0, -60.0], [59.0, -58.0]]       # no member inside anywhere
    return _frozen(Scene(_field(rng, h, w, holes=0.03), _swirl(h, w, h, w, 1.7), _dense(h, w), (0.5, 1.0, 2.0), shifts,
                         np.array([5.0, 20.0, 35.0], np.float32), 2, "nearest", min_members))


@functools.lru_cache(maxsize=None)
def caps() -> Scene:
    rng = np.random.default_rng(202)
    h, w = 20, 70
    src = _field(rng, h, w, holes=0.02)
    src[4:16, 20:50] = np.float32(63.0)                                      # a block every member lands in
    leads = tuple(0.25 * (k + 1) for k in range(16))
    shifts = rng.uniform(-2.0, 2.0, size=(16, 64, 2))
    return _frozen(Scene(src, _swirl(h, w, h, w, 0.6), _dense(h, w), leads, shifts,
                         np.array([-4.0, 0.0, 10.0, 18.0, 30.0, 35.0, 45.0, 62.5], np.float32), 16, "bilinear", 1))


@functools.lru_cache(maxsize=None)
def ties() -> Scene:
    rng = np.random.default_rng(303)
    h, w = 23, 41
    thr = np.array([0.0, 18.0, 35.0, 45.5], np.float32)
    palette = np.array([0.0, -0.0, 18.0, 35.0, 45.5, np.inf, -np.inf, np.nan, np.nextafter(np.float32(18.0), np.float32(0.0)),
                        np.nextafter(np.float32(35.0), np.float32(99.0)), 7.25, 50.0], np.float32)
    src = palette[rng.integers(0, len(palette), size=(h, w))]
    shifts = np.round(rng.uniform(-6.0, 6.0, size=(2, 6, 2)) * 2.0) / 2.0      # whole and half pixels
    return _frozen(Scene(src, _swirl(h, w, h, w, 1.1), _dense(h, w), (0.0, 1.5), shifts, thr, 1, "nearest", 2))


@functools.lru_cache(maxsize=None)
def lattice() -> Scene:
    rng = np.random.default_rng(404)
    h, w = 70, 129
    lat = mo.Lattice(5.5, 7.5, 29.5, 38.0, 3, 4)
    return _frozen(Scene(_field(rng, h, w, holes=0.10), _swirl(h, w, 3, 4, 2.3), lat, (1.0, 2.5, -0.75),
                         rng.uniform(-4.0, 4.0, size=(3, 7, 2)), np.array([10.0, 25.0, 40.0], np.float32), 3, "bilinear", 3))


@functools.lru_cache(maxsize=None)
def slivers():
    """((h, w), method) -> Scene for 1 x 1, 1 x 200 and 200 x 1, both methods."""
    out = {}
    for n, (h, w) in enumerate(((1, 1), (1, 200), (200, 1))):
        for method in ("nearest", "bilinear"):
            rng = np.random.default_rng(500 + n)
            shifts = rng.uniform(-1.2, 1.2, size=(2, 3, 2))
            shifts[:, 0] = 0.0
            out[(h, w), method] = _frozen(Scene(_field(rng, h, w, holes=0.05 if h * w > 1 else 0.0), _swirl(h, w, h, w, 0.4),
                                                _dense(h, w), (0.0, 1.0), shifts, np.array([0.0, 20.0], np.float32), 1, method, 1))
    return out


def _hist_inputs(rng, n, h, w, M, T, p_incomplete=0.1, p_nan=0.05, masked=0.1):
    counts = rng.integers(0, M + 1, size=(n, T, h, w)).astype(np.uint8)
    members = np.where(rng.random((n, h, w)) < p_incomplete, rng.integers(0, M, size=(n, h, w)), M).astype(np.uint8)
    obs = rng.uniform(-5.0, 60.0, size=(n, h, w)).astype(np.float32)
    obs[rng.random((n, h, w)) < p_nan] = np.nan
    mask = (rng.random((n, h, w)) < masked).astype(np.uint8) * rng.integers(1, 256, size=(n, h, w)).astype(np.uint8) if masked else None
    return counts, members, obs, mask


@functools.lru_cache(maxsize=None)
def trips() -> HistScene:
    rng = np.random.default_rng(606)
    per_trip = HIST_MAX_STRIPS * BLOCK
    h = 300
    w = per_trip // h + 63                                                   # a little more than one trip, no multiple of 64
    thr = np.array([18.0, 35.0, 45.0], np.float32)
    return _frozen(HistScene(*_hist_inputs(rng, 1, h, w, 20, 3), 20, thr))


@functools.lru_cache(maxsize=None)
def many_planes() -> HistScene:
    rng = np.random.default_rng(707)
    return _frozen(HistScene(*_hist_inputs(rng, 4099, 2, 3, 3, 2, masked=0.0), 3, np.array([10.0, 30.0], np.float32)))


@functools.lru_cache(maxsize=None)
def planted() -> HistScene:
    rng = np.random.default_rng(808)
    M = 11
    counts, members, obs, mask = _hist_inputs(rng, 3, 19, 67, M, 4, p_incomplete=0.0, p_nan=0.0, masked=0.0)
    counts[0, 1, 3, 5:9] = (M + 1, 200, 255, 64)                             # above M at ONE threshold of the pixel
    counts[2, :, 10, 20] = 255
    members[1, 4, 7:10] = (M - 1, 0, 255)                                    # incomplete, empty, overfull
    members[2, 18, 66] = M + 1
    obs[1, 0, 0] = obs[2, 5, 5] = np.nan
    obs[0, 2, 2], obs[0, 2, 3] = np.inf, -np.inf                             # values
    mask = np.zeros(obs.shape, np.uint8)
    mask[0, 6, 1:4] = (1, 128, 255)
    return _frozen(HistScene(counts, members, obs, mask, M, np.array([0.0, 18.0, 35.0, 45.0], np.float32)))


HIST_SCENES = dict(trips=trips, many_planes=many_planes, planted=planted)


def field_scenes():
    """name -> Scene of everything that goes through rg_ensemble_exceedance_f32."""
    out = {"rim-min1": rim(1), "rim-min5": rim(5), "caps": caps(), "ties": ties(), "lattice": lattice()}
    out.update({f"sliver-{h}x{w}-{method}": s for ((h, w), method), s in slivers().items()})
    return out


@functools.lru_cache(maxsize=None)
def expected(name) -> eo.Exceedance:
    s = field_scenes()[name]
    out = eo.exceedance(s.src, s.motion, s.lattice, s.leads, s.shifts, s.thresholds, s.substeps, s.method, s.min_members)
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def expected_hist(name):
    s = HIST_SCENES[name]()
    return _frozen(eo.histogram(s.counts, s.members, s.obs, s.mask, s.n_members, s.thresholds))


def observed_for(name) -> np.ndarray:
    """float32 [L, h, w]: an observation for a field scene -- the source moved a little, with holes of its own."""
    s = field_scenes()[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    obs = np.stack([np.roll(s.src, (l + 1, -l), axis=(0, 1)) for l in range(len(s.leads))]).astype(np.float32)
    obs[rng.random(obs.shape) < 0.04] = np.nan
    return obs
