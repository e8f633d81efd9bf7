"""Scenes for the cell kernels (csrc/rg_components.hip, csrc/rg_tracking.hip) at the sizes where a trip count or a magnitude
depends on size -- what tests/component_scenes.py and tests/tracking_scenes.py, which stop at 69 x 199, never reach:

``many_planes``   600 planes of 2 x 3: one chunk per plane, three trips of ``cc_scan_kernel`` with a ``cell_ptr`` entry written
                  in every trip, and about ten plane boundaries inside one wavefront, usually with label 1 on both sides;
``straddle``      90 planes of (TH + 1) x (TW + 1): three chunks per plane, so chunk 256 -- where the scan's second trip
                  starts -- lies in the middle of a plane;
``one_big``       one plane of (16 TH + 8) x (8 TW + 5): more than 256 chunks, 153 tiles, ragged both ways, with the patterns
                  of component_scenes.py (same generators, same seeds by name and shape);
``long_row`` / ``long_column``   1 x 100 000 and 100 000 x 1, whole and with one pixel cut out: index sums above 2^32, and
                  answers that are closed forms (:func:`line_expected`), no flood fill.

Every shape follows from the tile constants and from ``kBlock`` / ``kPerThread``, which are read from the kernel sources.
Scenes are ``component_scenes.Scene``; everything is deterministic (crc32-seeded) and importable without a GPU."""
import functools
import math
import os
import re

import numpy as np

import component_scenes as cs
import components_oracle as co
import tracking_scenes as ts

TH, TW = cs.TH, cs.TW
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "radar_processor_amd", "csrc")


def _constant(source, name):
    """``constexpr int <name> = <integer>;`` of a kernel source, or None when the line is not there."""
    with open(os.path.join(_CSRC, source)) as f:
        found = re.search(r"^\s*constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, f.read(), flags=re.M)
    return int(found.group(1)) if found else None


BLOCK = _constant("rg_common.hpp", "kBlock")                   # threads of a workgroup: chunk counts per scan trip
PER_THREAD = _constant("rg_components.hip", "kPerThread")      # consecutive pixels of one thread in flatten / rank
CHUNK = BLOCK * PER_THREAD if BLOCK and PER_THREAD else None   # pixels of one chunk: the unit of the scan
LO = cs.LO

MANY_PLANES = 2 * (BLOCK or 0) + 88                            # 600: two full scan trips and a ragged third
MANY_SHAPE = (2, 3)
STRADDLE_PLANES = 90
STRADDLE_SHAPE = (TH + 1, TW + 1)
BIG = (16 * TH + 8, 8 * TW + 5)
LINE = 100_000
CUT = 70_001
PEAK = 70.0
PEAKS = (12_345, 60_000, 80_000, LINE - 1)                     # the maximum twice in every cell of a cut line: ties
SHIFT = (2, -3)


def chunks_of(shape3):
    """Chunks of one call: ``n * ceil(h * w / CHUNK)``, the trip count of the scan's input."""
    n, h, w = shape3
    return n * (-(-h * w // CHUNK))


def scan_trips(shape3):
    return -(-chunks_of(shape3) // BLOCK)


# ---- patterns ---------------------------------------------------------------------------------------------------------------
def _many_pattern(name):
    pattern = cs._rng(name, MANY_SHAPE).random((MANY_PLANES,) + MANY_SHAPE) < 0.5
    pattern[::7] = False                                        # every 7th plane is empty: equal cell_ptr entries in a row
    pattern[0] = pattern[-1] = True                             # foreground on the first and on the last pixel of the call
    return pattern


def _scene(name, pattern, wrap=False, dress=None):
    pattern = np.asarray(pattern, bool)
    pattern = pattern[None] if pattern.ndim == 2 else pattern
    planes = cs._dress(dress or name, pattern)
    planes.setflags(write=False)
    return cs.Scene(name, planes, LO, np.inf, None, wrap)


def _line(name, shape, cut, wrap=False):
    """All foreground on a ramp of the 0.5 dB lattice, the maximum at PEAKS; ``cut``: pixel CUT is NaN."""
    i = np.arange(LINE)
    v = (LO + 0.5 * (i % 50)).astype(np.float32)
    v[list(PEAKS)] = PEAK
    if cut:
        v[CUT] = np.nan
    planes = v.reshape((1,) + shape)
    planes.setflags(write=False)
    return cs.Scene(name, planes, LO, np.inf, None, wrap)


@functools.lru_cache(maxsize=None)
def scenes():
    h, w = BIG
    yy, xx = np.mgrid[0:h, 0:w]
    out = [_scene("many_planes", _many_pattern("many_planes")),
           _scene("many_planes_wrap", _many_pattern("many_planes"), wrap=True, dress="many_planes"),
           _scene("straddle", cs._rng("straddle", STRADDLE_SHAPE).random((STRADDLE_PLANES,) + STRADDLE_SHAPE) < 0.45)]
    for d in (0.41, 0.593):
        out.append(_scene(f"random_{d}", cs._rng(f"random_{d}", BIG).random(BIG) < d))
    out += [_scene("serpentine", cs.serpentine(h, w)), _scene("comb", cs.comb(h, w)),
            _scene("all_foreground", np.ones(BIG, bool)), _scene("checkerboard", (yy + xx) % 2 == 0),
            _scene("wrap_random_0.45", cs._rng("wrap_random", BIG).random(BIG) < 0.45, wrap=True),
            _scene("wrap_serpentine", cs.serpentine(h, w), wrap=True),
            _line("long_row", (1, LINE), False), _line("long_row_cut", (1, LINE), True),
            _line("long_column", (LINE, 1), False), _line("long_column_cut", (LINE, 1), True),
            _line("long_column_cut_wrap", (LINE, 1), True, wrap=True)]
    return tuple(out)


def scene(name):
    return next(s for s in scenes() if s.name == name)


# (scene, connectivity) in the order the GPU tests run them: the smallest input that takes a second scan trip comes first
MANY_CASES = tuple((name, c) for name in ("many_planes", "many_planes_wrap") for c in (4, 8))
STRADDLE_CASES = (("straddle", 4), ("straddle", 8))
BIG_CASES = (("random_0.41", 8), ("random_0.593", 4), ("serpentine", 4), ("comb", 8), ("all_foreground", 8), ("checkerboard", 4),
             ("wrap_random_0.45", 8), ("wrap_serpentine", 4))
LONG_CASES = tuple((name, c) for name in ("long_row", "long_row_cut", "long_column", "long_column_cut", "long_column_cut_wrap")
                   for c in (4, 8))
CASES = MANY_CASES + STRADDLE_CASES + BIG_CASES + LONG_CASES
# the cases whose whole table goes through components_oracle.stats (a Python loop per cell and per pixel)
FULL_TABLE_CASES = MANY_CASES + STRADDLE_CASES + (("random_0.41", 8), ("serpentine", 4), ("all_foreground", 8))
DESPECKLE_CASES = MANY_CASES + STRADDLE_CASES + (("random_0.41", 8),)


def case_id(case):
    return f"{case[0]}-c{case[1]}"


# ---- references -------------------------------------------------------------------------------------------------------------
def line_cells(name):
    """The cells of a ``long_*`` scene as lists of (first, last) index ranges, in label order."""
    if not name.startswith("long_"):
        raise KeyError(name)
    if "cut" not in name:
        return [[(0, LINE - 1)]]
    if name.endswith("wrap"):
        return [[(0, CUT - 1), (CUT + 1, LINE - 1)]]            # the column's two ends meet across the wrap seam
    return [[(0, CUT - 1)], [(CUT + 1, LINE - 1)]]


def line_expected(name):
    """``(labels, cell_ptr, table)`` of a ``long_*`` scene without a flood fill: index arithmetic in int64.  The table has
    the columns of ``components_oracle.stats``."""
    s = scene(name)
    v = s.planes.ravel()
    column = s.planes.shape[2] == 1
    cells = line_cells(name)
    labels = np.zeros(LINE, np.int32)
    keys = ("plane", "id", "area", "bbox", "sum_yx", "vmax", "argmax", "vsum", "abs_sum")
    rows = {k: [] for k in keys}
    for k, ranges in enumerate(cells, 1):
        idx = np.concatenate([np.arange(a, b + 1, dtype=np.int64) for a, b in ranges])
        labels[idx] = k
        total, zero = int(idx.sum()), 0
        span = [int(idx.min()), int(idx.max()), 0, 0]
        rows["plane"].append(0), rows["id"].append(k), rows["area"].append(len(idx))
        rows["bbox"].append(span if column else span[2:] + span[:2])
        rows["sum_yx"].append([total, zero] if column else [zero, total])
        rows["vmax"].append(v[idx].max()), rows["argmax"].append(int(idx[np.argmax(v[idx])]))       # the first of the ties
        rows["vsum"].append(math.fsum(v[idx].astype(np.float64))), rows["abs_sum"].append(math.fsum(np.abs(v[idx]).astype(np.float64)))
    dtypes = dict(plane=np.int32, id=np.int32, area=np.int32, bbox=np.int32, sum_yx=np.int64, vmax=np.float32, argmax=np.int32,
                  vsum=np.float64, abs_sum=np.float64)
    table = {k: np.array(rows[k], dtype=dtypes[k]) for k in keys}
    return labels.reshape(s.planes.shape), np.array([0, len(cells)], np.int32), table


@functools.lru_cache(maxsize=None)
def labelled(name, connectivity):
    """``(labels, cell_ptr)``: the closed form for ``long_*``, the oracle's flood fill for everything else.  Read-only."""
    s = scene(name)
    if name.startswith("long_"):
        labels, cell_ptr, _ = line_expected(name)
    else:
        labels, cell_ptr = co.label(s.planes, s.lo, s.hi, s.mask, connectivity, s.wrap)
    labels.setflags(write=False), cell_ptr.setflags(write=False)
    return labels, cell_ptr


def vector_table(planes, labels, cell_ptr):
    """``area``, ``bbox``, ``sum_yx``, ``vmax``, ``argmax``, ``plane`` and ``id`` of a labelling in vectorised NumPy, for
    scenes with far too many cells for ``components_oracle.stats``.  Exact: integer columns in int64 arithmetic; ``vmax`` by
    ``np.maximum.at`` over values that hold no NaN and no zero inside a cell (asserted), so the numeric order is the total
    order."""
    planes, labels = np.asarray(planes, np.float32), np.asarray(labels)
    n, h, w = planes.shape
    ptr = np.asarray(cell_ptr, np.int64)
    cells = int(ptr[-1])
    p, y, x = np.nonzero(labels)
    row = ptr[p] + labels[p, y, x] - 1
    v = planes[p, y, x]
    assert not np.isnan(v).any() and (v != 0).all()
    flat = y.astype(np.int64) * w + x
    out = dict(area=np.bincount(row, minlength=cells).astype(np.int32), bbox=np.empty((cells, 4), np.int32),
               sum_yx=np.zeros((cells, 2), np.int64), vmax=np.full(cells, -np.inf, np.float32))
    for col, (a, fn, start) in enumerate(((y, np.minimum, h), (y, np.maximum, -1), (x, np.minimum, w), (x, np.maximum, -1))):
        best = np.full(cells, start, np.int64)
        fn.at(best, row, a)
        out["bbox"][:, col] = best
    np.add.at(out["sum_yx"][:, 0], row, y.astype(np.int64))
    np.add.at(out["sum_yx"][:, 1], row, x.astype(np.int64))
    np.maximum.at(out["vmax"], row, v)
    first = np.full(cells, h * w, np.int64)
    at_peak = v == out["vmax"][row]
    np.minimum.at(first, row[at_peak], flat[at_peak])
    out["argmax"] = first.astype(np.int32)
    out["plane"] = (np.searchsorted(ptr[1:], np.arange(cells), side="right")).astype(np.int32)
    out["id"] = (np.arange(cells) - ptr[out["plane"]] + 1).astype(np.int32)
    return out


# ---- pairs of label stacks for the overlap kernels -----------------------------------------------------------------------------
def _label_pattern(pattern, connectivity=8):
    pattern = np.asarray(pattern, bool)
    pattern = pattern[None] if pattern.ndim == 2 else pattern
    return co.label(np.where(pattern, np.float32(40.0), np.float32(np.nan)), LO, connectivity=connectivity)


def _foreground(name):
    s = scene(name)
    return co.foreground(s.planes, s.lo, s.hi, s.mask)


@functools.lru_cache(maxsize=None)
def overlap_scenes():
    """``tracking_scenes.Scene`` pairs: many planes against another seed's; a big random plane against itself moved by
    SHIFT; 134 000 one-pixel cells that all share one next cell; a long row against its cut variant."""
    out = [ts.Scene("many_planes", *labelled("many_planes", 8), *_label_pattern(_many_pattern("many_planes_other"))),
           ts.Scene("random_0.41_shifted", *labelled("random_0.41", 8),
                    *_label_pattern(ts.shifted(_foreground("random_0.41")[0], *SHIFT))),
           ts.Scene("checker_vs_all", *labelled("checkerboard", 4), *labelled("all_foreground", 8)),
           ts.Scene("long_row_vs_cut", *labelled("long_row", 8), *labelled("long_row_cut", 8))]
    for s in out:
        for a in s[1:]:
            a.setflags(write=False)
    return tuple(out)


def overlap_scene(name):
    return next(s for s in overlap_scenes() if s.name == name)


OVERLAP_NAMES = ("many_planes", "random_0.41_shifted", "checker_vs_all", "long_row_vs_cut")
