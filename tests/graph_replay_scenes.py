"""Pairs of inputs for the capture-and-replay tests (tests/test_graph_replay_scenes.py, tests/test_gpu_graph_replay.py).

A chain is captured into a graph on inputs A and replayed on inputs B in the same buffers.  A and B of a chain have the same
shapes, dtypes and host-side parameters (thresholds, scales, radii, lattices, ``max_pairs``), so the host code of every entry
point takes the same path and the captured launch geometry holds for both; only device data differs.  They are two scenes of
one shape from the family's own scene module where it has them (``main_35`` / ``main_39``),
otherwise the family's generator with other seeds, or A flipped along both axes and rolled.

No oracle is written here: ``expected(chain, which)`` calls the family's restatement (tests/*_oracle.py and the
``expected()`` of the scene modules) and returns ``{output name: array}``.  Everything is computed once, shared and
read-only."""
from __future__ import annotations

import functools
from typing import Dict, NamedTuple, Tuple

import numpy as np

from oracle import radar_grid_oracle as oracle

import accumulation_oracle as ao
import accumulation_scenes as acs
import closest_scenes as cls
import combine_scenes as cbs
import component_scenes as cs
import column_profile_oracle as cpo
import components_oracle as cco
import convection_scenes as cvs
import georef_oracle as go
import motion_oracle as mo
import mosaic_section_scenes as mss
import motion_scenes as ms
import product_scenes as ps
import section_scenes as ss
import slab_scenes as sl
import tracking_oracle as to
import tracking_scenes as ts
import verification_oracle as vo
import verification_scenes as vs
import warp_oracle as wo

CHAINS = ("verification", "convection", "tracking", "raster", "accumulation", "motion", "cells", "products", "georef", "gridding", "columns", "mosaic", "prologue")
WHICH = ("A", "B")


def flipped_and_rolled(a, axes, roll):
    """``a`` reversed along ``axes`` and then rolled by ``roll`` along them: every element moves."""
    return np.ascontiguousarray(np.roll(np.flip(a, axes), roll, axes))


def _frozen(arrays: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    for a in arrays.values():
        a.setflags(write=False)
    return arrays


# ---- verification: the shape, thresholds and scales of verification_scenes' "rows", drawn with other seeds ---------------------
VERIFICATION_SEEDS = {"A": (5, 6, 11), "B": (105, 106, 111)}      # A is "rows" itself


@functools.lru_cache(maxsize=None)
def verification(which: str) -> vs.Scene:
    rows = vs.scene("rows")
    if which == "A":
        return rows
    shape = rows.forecast.shape
    f_seed, o_seed, m_seed = VERIFICATION_SEEDS[which]
    rng = np.random.default_rng(m_seed)
    mask = (rng.random(shape) < 0.03).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)
    s = vs.Scene("rows_b", vs.levels(shape, f_seed, vs.ROWS_LEVELS, 0.05), vs.levels(shape, o_seed, vs.ROWS_LEVELS, 0.05), mask,
                 rows.thresholds, rows.scales)
    for a in (s.forecast, s.observed, s.mask):
        a.setflags(write=False)
    return s


def verification_ends(s: vs.Scene) -> Tuple[int, int]:
    """The two window sizes of the fraction planes: the smallest and the largest of the ladder."""
    return s.scales[0], s.scales[-1]


def _verification_expected(which):
    s = verification(which)
    c = vo.contingency(s.forecast, s.observed, s.thresholds, s.mask)
    sat_f = vo.sat(s.forecast, s.thresholds, s.observed, s.mask)
    return dict(counts=c.counts, valid=c.valid, sat_f=sat_f, sat_o=vo.sat(s.observed, s.thresholds, s.forecast, s.mask),
                sums=vo.fss_sums(s.forecast, s.observed, s.thresholds, s.scales, s.mask),
                frac=np.stack([vo.box_fraction(sat_f, n) for n in verification_ends(s)]).astype(np.float32))


# ---- convection: the two main scenes ---------------------------------------------------------------------------------------------
CONVECTION = dict(zip(WHICH, cvs.MAIN))


def convection(which: str) -> cvs.Scene:
    return cvs.scene(CONVECTION[which])


def _convection_expected(which):
    want = cvs.expected(CONVECTION[which])
    return dict(q=want.q, flag=want.echo.astype(np.int32), S=want.S, N=want.N, bkg=want.bkg, centres=want.centres,
                classes=want.classes)


# ---- tracking: tracking_scenes' smoothed noise on 45 x 150, and the same patterns flipped and rolled -----------------------------
# The module's own pairs of one shape below 69 x 199 (the checkerboards) share their labels_prev, so the static input would not
# change between A and B; its generator at a smaller shape gives label sets that differ in both frames.
TRACK_SHAPE = (45, 150)
TRACK_LEVEL = 0.55
TRACK_ROLL = (7, 31)
TRACK_MAX_PAIRS = 128             # explicit, holds both scenes (asserted on the CPU); the table has 256 slots
TRACK_CELLS = 128                 # n_cells of the relabel calls and the length of the table: covers both scenes


@functools.lru_cache(maxsize=None)
def tracking(which: str) -> ts.Scene:
    prev = ts.smooth_noise("blobs", TRACK_SHAPE) >= TRACK_LEVEL
    nxt = ts.shifted(prev, 2, -3)
    if which == "B":
        prev, nxt = (flipped_and_rolled(p, (0, 1), TRACK_ROLL) for p in (prev, nxt))
    s = ts.Scene("replay_" + which, *ts._label(prev), *ts._label(nxt))
    for a in s[1:]:
        a.setflags(write=False)
    return s


def track_lut(n=TRACK_CELLS) -> np.ndarray:
    """The table of tests/test_gpu_tracking.py: any integers, negative too."""
    return (np.arange(n, dtype=np.int64) * 2654435761 % 1000003 - 500000).astype(np.int32)


def _tracking_expected(which):
    s = tracking(which)
    rows_prev, rows_next, count = to.overlap(s.labels_prev, s.ptr_prev, s.labels_next, s.ptr_next)
    return dict(pairs=np.stack([rows_prev, rows_next, count], axis=1),                 # sorted by (row_prev, row_next)
                relabel_prev=to.relabel(s.labels_prev, s.ptr_prev, track_lut()),
                relabel_next=to.relabel(s.labels_next, s.ptr_next, track_lut()))     # computed in place on the device


def overlap_capacity(max_pairs: int) -> int:
    """The smallest power of two that is at least ``max(2 * max_pairs, 64)`` (header: rg_cell_overlap_workspace_bytes)."""
    c = 64
    while c < 2 * max_pairs:
        c *= 2
    return c


def overlap_home_slot(row_prev: int, row_next: int, capacity: int) -> int:
    """The slot a pair is first looked for: the finaliser of splitmix64 on ``(row_prev << 32) | row_next``, masked."""
    m = (1 << 64) - 1
    k = ((row_prev << 32) | row_next) & m
    k ^= k >> 30
    k = k * 0xBF58476D1CE4E5B9 & m
    k ^= k >> 27
    k = k * 0x94D049BB133111EB & m
    k ^= k >> 31
    return k & (capacity - 1)


def overlap_slots(pairs, max_pairs: int) -> frozenset:
    """The slots the pairs occupy after linear probing.  The occupied set of a linear-probing table does not depend on the
    order of insertion, so the sorted order stands for whichever order the device takes."""
    capacity = overlap_capacity(max_pairs)
    held = set()
    for a, b in np.asarray(pairs)[:, :2].tolist():
        slot = overlap_home_slot(a, b, capacity)
        while slot in held:
            slot = (slot + 1) & (capacity - 1)
        held.add(slot)
    return frozenset(held)


# ---- raster: warp_oracle's "rma1_fine"; the geometry is host-side, the sources differ --------------------------------------------
RASTER_SCENE = "rma1_fine"
RASTER_ROLL = (5, 11)
RASTER_FACTOR = 4                 # of the float overviews
RASTER_FACTOR_RGBA = 2
RASTER_BILINEAR_KIND = "nan_30_percent"
COLORMAP = (2000.0, 30000.0, 256, 7)       # vmin, vmax, entries and seed of product_scenes.random_lut; no fill value: NaN is no-data


def colormap_lut() -> np.ndarray:
    return ps.random_lut(COLORMAP[2], COLORMAP[3])


@functools.lru_cache(maxsize=None)
def raster(which: str) -> Dict[str, np.ndarray]:
    """``planes`` float32 [3, ny, nx] for the nearest warp, ``plane`` float32 [1, ny, nx] for the bilinear one, ``rgba``."""
    out = dict(planes=np.array(wo.planes(RASTER_SCENE, 3)), plane=np.array(wo.bilinear_source(RASTER_SCENE, RASTER_BILINEAR_KIND))[None],
               rgba=wo.index_rgba(wo.scene(RASTER_SCENE).shape))
    if which == "B":
        out = dict(planes=flipped_and_rolled(out["planes"], (1, 2), RASTER_ROLL), plane=flipped_and_rolled(out["plane"], (1, 2), RASTER_ROLL),
                   rgba=flipped_and_rolled(out["rgba"], (0, 1), RASTER_ROLL))
    return _frozen(out)


def _raster_expected(which):
    s, src = wo.scene(RASTER_SCENE), raster(which)
    fx, fy, c = wo.mapped(RASTER_SCENE)
    near = wo.sample_nearest(src["planes"], fx, fy, c, s.lattice, np.float32(np.nan))
    bil = wo.sample_bilinear(src["plane"][0], fx, fy, c, s.lattice, np.nan)[0].astype(np.float32)[None]
    rgba = wo.sample_nearest(src["rgba"], fx, fy, c, s.lattice, 0)
    coloured = ps.colormap_reference(src["plane"][0], COLORMAP[0], COLORMAP[1], colormap_lut())
    return dict(near=near, near_overview=np.ascontiguousarray(wo.overview_nearest(near, RASTER_FACTOR)), bilinear=bil,
                bilinear_overview=wo.overview_average(bil, RASTER_FACTOR).astype(np.float32), rgba=rgba,
                rgba_overview=np.ascontiguousarray(wo.overview_nearest(rgba, RASTER_FACTOR_RGBA)), coloured=coloured,
                coloured_warped=wo.sample_nearest(coloured, fx, fy, c, s.lattice, 0))


# ---- accumulation: the shape, lattice and parameters of "dense_bilinear" and of "dense_nearest" -------------------------------
# The planes of the family's generator are read as dBZ here (0 .. 90 with NaN and +inf: dry, wet, capped and missing pixels), so
# that rg_rain_rate_f32 feeds the accumulation inside one graph.
ACCUMULATION_SEEDS = {"A": (5, 6, 7), "B": (105, 106, 107)}       # A: the planes and the field of "dense_bilinear"
ZR = (200.0, 1.6, 5.0, 55.0)      # a, b, min_dbz, max_dbz


class AccumulationScene(NamedTuple):
    dbz_prev: np.ndarray          # float32 [3, 37, 53]
    dbz_next: np.ndarray
    motion: np.ndarray            # float32 [37, 53, 2]
    bilinear: acs.Scene           # the parameters of "dense_bilinear" (its planes are not used)
    nearest: acs.Scene            # the parameters of "dense_nearest"


@functools.lru_cache(maxsize=None)
def accumulation(which: str) -> AccumulationScene:
    bil, near = acs.scene("dense_bilinear"), acs.scene("dense_nearest")
    assert tuple(bil.lattice) == tuple(near.lattice) and bil.hours == near.hours
    p_seed, n_seed, m_seed = ACCUMULATION_SEEDS[which]
    shape = bil.prev.shape[1:]
    s = AccumulationScene(acs.rates(shape, 3, p_seed, True), acs.rates(shape, 3, n_seed, True), acs.fractional(bil.lattice, m_seed), bil,
                          near)
    for a in s[:3]:
        a.setflags(write=False)
    return s


def accumulation_from_rates(s: AccumulationScene, rate_prev, rate_next):
    """Both accumulations by the restatement from given rate planes: ``(bilinear, nearest)`` as ``ao.Accumulation``."""
    return tuple(ao.accumulate(rate_prev, rate_next, s.motion, p.lattice, p.hours, p.n_steps, p.substeps, p.method, p.min_steps, p.fill)
                 for p in (s.bilinear, s.nearest))


def _accumulation_expected(which):
    s = accumulation(which)
    rate_prev, rate_next = (ao.rain_rate(d, *ZR) for d in (s.dbz_prev, s.dbz_next))
    bil, near = accumulation_from_rates(s, rate_prev, rate_next)
    return dict(rate_prev=rate_prev, rate_next=rate_next, depth_bilinear=bil.out, steps_bilinear=bil.steps, depth_nearest=near.out,
                steps_nearest=near.steps)


# ---- motion: "shift", and "subpixel" flipped and rolled ------------------------------------------------------------------------
# The two scenes share their earlier plane (one field, two displacements), so B is turned over: both of its planes differ from A's.
MOTION_ROLL = (9, 17)
ADVECT_LEADS = (1.0, 2.5)
ADVECT_SUBSTEPS = 2
ADVECT_FILL = -9.25


@functools.lru_cache(maxsize=None)
def motion(which: str) -> ms.Scene:
    if which == "A":
        return ms.scene("shift")
    sub = ms.scene("subpixel")
    s = sub._replace(name="subpixel_turned", prev=flipped_and_rolled(sub.prev, (0, 1), MOTION_ROLL),
                     next=flipped_and_rolled(sub.next, (0, 1), MOTION_ROLL), truth=None)
    for a in (s.prev, s.next):
        a.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def motion_match(which: str):
    """``(q_prev, q_next, Match)`` by the restatement, as ``motion_scenes.levels`` and ``motion_scenes.match`` form them."""
    s = motion(which)
    q_prev, q_next = mo.quantize(s.prev, ms.LO, ms.HI, None), mo.quantize(s.next, ms.LO, ms.HI, None)
    return q_prev, q_next, mo.block_match(q_prev, q_next, s.B, s.S, s.R, s.min_echo)


@functools.lru_cache(maxsize=None)
def motion_field(which: str):
    """``(field float32 [nby, nbx, 2], lattice)``: the scene's restated match with its gaps filled, as the nowcast takes it."""
    s, m = motion(which), motion_match(which)[2]
    field = np.ascontiguousarray(mo.fill_motion(m.motion[0], m.score[0]), dtype=np.float32)
    field.setflags(write=False)
    return field, mo.block_lattice(s.prev.shape, s.B, s.S)


def _motion_expected(which):
    s = motion(which)
    q_prev, q_next, m = motion_match(which)
    field, lat = motion_field(which)
    out = dict(q_prev=q_prev[None], q_next=q_next[None], disp=m.disp, motion=m.motion.astype(np.float32), score=m.score.astype(np.float32))
    for method in ("nearest", "bilinear"):
        out["advect_" + method] = mo.advect(s.prev[None], field, lat, ADVECT_LEADS, ADVECT_SUBSTEPS, method, ADVECT_FILL)
    return out


# ---- cells: two planes of component_scenes' largest shape, connectivity 8, with a mask -----------------------------------------------
# The module has no scene of two planes with a mask, so each of A and B stacks two of its random scenes (one threshold, lo = 35)
# under a mask drawn here.  One tile column of A's second plane and one tile row of B's first are blanked, so that the two
# leave foreground -- and with it parents and chunk counts in the workspace -- in different tiles.
CELLS_SHAPE = cs.SHAPES[-1]                            # (2 * TH + 5, 3 * TW + 7)
CELLS_SOURCES = {"A": ("random_0.41", "random_0.45"), "B": ("random_0.593", "random_0.3")}
CELLS_MASK_SEEDS = {"A": 41, "B": 59}
CELLS_CONNECTIVITY = 8
CELLS_BOUND = 1024                # n_cells of the table call: covers both scenes (asserted on the CPU)
CELLS_MIN_SIZE, CELLS_FILL = 3, -9.25


class CellScene(NamedTuple):
    planes: np.ndarray            # float32 [2, h, w]
    mask: np.ndarray              # uint8 [2, h, w]
    lo: float
    hi: float


@functools.lru_cache(maxsize=None)
def cells(which: str) -> CellScene:
    first, second = (cs.scene(CELLS_SHAPE, name) for name in CELLS_SOURCES[which])
    assert (first.lo, first.hi, first.wrap) == (second.lo, second.hi, second.wrap) == (cs.LO, np.inf, False)
    planes = np.concatenate([first.planes, second.planes]).copy()
    if which == "A":
        planes[1, :, :cs.TW] = np.nan
    else:
        planes[0, :cs.TH, :] = np.nan
    rng = np.random.default_rng(CELLS_MASK_SEEDS[which])
    mask = (rng.random(planes.shape) < 0.1).astype(np.uint8) * rng.integers(1, 256, planes.shape).astype(np.uint8)
    planes.setflags(write=False)
    mask.setflags(write=False)
    return CellScene(planes, mask, cs.LO, np.inf)


@functools.lru_cache(maxsize=None)
def cells_reference(which: str):
    """``(labels, cell_ptr, table)`` by the flood-fill restatement, as tests/test_gpu_components.py forms them."""
    s = cells(which)
    labels, cell_ptr = cco.label(s.planes, s.lo, s.hi, s.mask, CELLS_CONNECTIVITY, False)
    table = cco.stats(s.planes, labels, cell_ptr)
    for a in (labels, cell_ptr, *table.values()):
        a.setflags(write=False)
    return labels, cell_ptr, table


def tiles_with_foreground(which: str) -> frozenset:
    """``(plane, tile row, tile column)`` of every tile of the labelling kernel that holds a foreground pixel."""
    labels = cells_reference(which)[0]
    p, y, x = np.nonzero(labels)
    return frozenset(zip(p.tolist(), (y // cs.TH).tolist(), (x // cs.TW).tolist()))


def _cells_expected(which):
    s = cells(which)
    labels, cell_ptr, table = cells_reference(which)
    out, removed = cco.despeckle_labelled(s.planes, labels, cell_ptr, CELLS_MIN_SIZE, CELLS_FILL)
    return dict(labels=labels, cell_ptr=cell_ptr, area=table["area"], bbox=table["bbox"], sum_yx=table["sum_yx"], vmax=table["vmax"],
                argmax=table["argmax"], vsum=table["vsum"], despeckled=out, removed=removed)


# ---- products: the stored grid of product_scenes' "from_limits_curved_steep" (7 x 5 x 259: six workgroups per plane) ----------------
PRODUCTS_SCENE = "from_limits_curved_steep"
PRODUCTS_LIMITS = ((7, 5, 259), ((500.0, 9500.0), (-30e3, 30e3), (-40e3, 40e3)), 19.5, True)      # the scene's own arguments
PRODUCTS_SEED_B = 111             # the scene's generator with another seed: a permuted grid would keep its minimum and maximum
PROFILE_THRESHOLDS = (18.0, 30.0)
PROFILE_MAX_DBZ = 56.0
COLLAPSE = (float(np.sin(np.deg2rad(2.5))), 2.0 * 8.49e6)       # sin_elev, two_re of tests/test_gpu_product_contracts.py
PLANE_TESTS = ((None, 0.0, 0.0, ps.RG_TEST_LO | ps.RG_TEST_NONFINITE), ("top", 2000.0, 0.0, ps.RG_TEST_LO))     # "top": the first echo-top plane
GRID_FILTER = (ps.RG_TEST_LO | ps.RG_TEST_HI | ps.RG_TEST_NONFINITE, -5.000001, 40.3, -9999.0)                  # flags, lo, hi, fill


@functools.lru_cache(maxsize=None)
def products(which: str) -> Dict[str, np.ndarray]:
    """``grid`` float32 [nz, ny, nx] and ``samples`` float32 [2, ny * nx]: the two levels the restated linear plan selects for
    every pixel, +inf where it selects none -- gathered on the host as tests/test_gpu_product_contracts.py gathers them."""
    s = ps.ppi_scene(PRODUCTS_SCENE)
    grid = np.array(s.grid)
    if which == "B":
        other = ps._from_limits("replay_b", *PRODUCTS_LIMITS, PRODUCTS_SEED_B)
        assert ps.ppi_scalars(other, True) == ps.ppi_scalars(s, True) and other.xc.tobytes() == s.xc.tobytes()
        assert other.yc.tobytes() == s.yc.tobytes() and other.grid.shape == grid.shape
        grid = np.array(other.grid)
    plan = ps.ppi_plan_reference(s, True)
    n = s.ny * s.nx
    flat = grid.reshape(s.nz, n)
    samples = np.stack([flat[plan.lo_s.ravel(), np.arange(n)], flat[plan.hi_s.ravel(), np.arange(n)]]).astype(np.float32)
    samples[:, ~plan.in_range.ravel()] = np.inf
    return _frozen(dict(grid=grid, samples=samples))


def products_levels() -> np.ndarray:
    """float64 [nz]: the height of every level of the scene's grid."""
    s = ps.ppi_scene(PRODUCTS_SCENE)
    return s.z_min + s.z_step * np.arange(s.nz, dtype=np.float64)


def products_tests(src, top):
    """``PLANE_TESTS`` as ``product_scenes.plane_filter_reference`` takes them."""
    return [(top if plane == "top" else None, lo, hi, flags) for plane, lo, hi, flags in PLANE_TESTS]


def _products_expected(which):
    s, grid = ps.ppi_scene(PRODUCTS_SCENE), products(which)["grid"]
    z, n = products_levels(), s.ny * s.nx
    top = np.stack([cpo.echo_top(grid, z, t, 0, s.nz - 1, True) for t in PROFILE_THRESHOLDS]).reshape(-1, n)
    base = np.stack([cpo.echo_base(grid, z, t, 0, s.nz - 1, True) for t in PROFILE_THRESHOLDS]).reshape(-1, n)
    plan = ps.ppi_plan_reference(s, True)
    ppi = ps.ppi_combine_reference(grid, plan, True).ravel()
    collapsed, level = ps.collapse_ppi_reference(grid, s.xc, s.yc, z, *COLLAPSE)
    masked, kept = ps.plane_filter_reference(collapsed.ravel(), None, products_tests(collapsed.ravel(), top[0]))
    flags, lo, hi, fill = GRID_FILTER
    filtered = ps.grid_filter_reference(grid, flags, lo, hi, None, fill)
    return dict(top=top, base=base, vil=cpo.vil(grid, z, PROFILE_MAX_DBZ, 0, s.nz - 1).ravel(), sel=plan.sel.ravel(), w_hi=plan.w_hi.ravel(),
                ppi=ppi, ppi_stored=ppi.copy(), collapsed=collapsed.ravel(), level=level.ravel(), kept=kept, kept_mask=masked.astype(np.uint8),
                filtered=filtered, minmax=ps.minmax_reference(filtered, fill))


# ---- georef: georef_oracle's "east_200km" gates, and the node tables of tests/test_gpu_georef.py -----------------------------------
GEOREF_SCENE = "east_200km"       # 4099 gates: seventeen workgroups
GEOREF_ROLL = 1501
NODE_SHAPE = (33, 47)
NODE_LIMITS = {"A": ((-310e3, 255e3), (-401e3, 377e3)), "B": ((-198e3, 333e3), (-287e3, 412e3))}      # A: the family test's


@functools.lru_cache(maxsize=None)
def georef(which: str) -> Dict[str, np.ndarray]:
    """``x``, ``y`` float32 [n] in the radar's plane; ``xc`` [nx], ``yc`` [ny] float32 node tables of a grid about the origin.
    The node tables are device arrays of rg_frame_to_lonlat_f64, not host-side parameters: the lattice of B is another one."""
    s = go.scene(GEOREF_SCENE)
    x, y = np.array(s.x), np.array(s.y)
    if which == "B":
        x, y = flipped_and_rolled(x, (0,), GEOREF_ROLL), flipped_and_rolled(y, (0,), GEOREF_ROLL)
    (y0, y1), (x0, x1) = NODE_LIMITS[which]
    return _frozen(dict(x=x, y=y, xc=np.linspace(x0, x1, NODE_SHAPE[1], dtype="float32"), yc=np.linspace(y0, y1, NODE_SHAPE[0], dtype="float32")))


def georef_placed(which: str):
    """``(x', y')`` float64 of the gates by the restatement, before the one rounding to float32."""
    s, d = go.scene(GEOREF_SCENE), georef(which)
    return go.place(d["x"], d["y"], s.radar, s.origin)[:2]


def _georef_expected(which):
    from radar_processor_amd import grid_to_geographic       # the host map tests/test_gpu_georef.py holds the node kernel to
    s, d = go.scene(GEOREF_SCENE), georef(which)
    px, py = georef_placed(which)
    lon, lat = grid_to_geographic(d["xc"][None, :].astype(np.float64), d["yc"][:, None].astype(np.float64), *s.origin)
    px32, py32 = px.astype(np.float32), py.astype(np.float32)
    return dict(x_frame=px32, y_frame=py32, x_in_place=px32.copy(), y_in_place=py32.copy(), lon=np.array(lon), lat=np.array(lat))


# ---- gridding: closest_scenes' "ties" (2 x 8 x 20 voxels: eight workgroups), three fields, a mask on two of them ---------------------
# The gates and the search built from them are geometry; the fields and their masks are the device data that differ.
GRIDDING_SCENE = "ties"
GRIDDING_FIELDS = 3
GRIDDING_WEIGHTING = "barnes2"


@functools.lru_cache(maxsize=None)
def gridding(which: str) -> Dict[str, np.ndarray]:
    """``f0 .. f2`` float32 [n_gates] and ``m0``, ``m2`` uint8 [n_gates] (field 1 has no mask).  A: the family's index-coded
    fields under the scene's own masks; B: seeded real values under other masks."""
    s = cls.scene(GRIDDING_SCENE)
    n = s.n_gates
    if which == "A":
        fields = [(np.arange(n, dtype=np.int64) + k * n).astype(np.float32) for k in range(GRIDDING_FIELDS)]
        masks = s.masks(GRIDDING_FIELDS)
    else:
        fields = [np.random.default_rng([s.seed, 19, k]).normal(20.0, 10.0, n).astype(np.float32) for k in range(GRIDDING_FIELDS)]
        masks = [np.random.default_rng([s.seed, 17, k]).random(n) < 0.25 if k % 2 == 0 else None for k in range(GRIDDING_FIELDS)]
    assert masks[1] is None and masks[0] is not None and masks[2] is not None
    out = {f"f{k}": f for k, f in enumerate(fields)}
    out.update({f"m{k}": masks[k].astype(np.uint8) for k in (0, 2)})
    return _frozen(out)


def gridding_masks(which: str):
    d = gridding(which)
    return [d["m0"] != 0, None, d["m2"] != 0]


@functools.lru_cache(maxsize=None)
def gridding_neighbours():
    """``(indptr, gate_indices, float64 weights)`` of the scene by the brute-force restatement."""
    s = cls.scene(GRIDDING_SCENE)
    return oracle.build_geometry(s.gx, s.gy, s.gz, s.shape, s.limits, radar_altitude=s.radar_altitude, min_radius=s.min_radius,
                                 beam_factor=s.beam_factor, weighting=GRIDDING_WEIGHTING, toa=s.toa, exact_weights=True)


def gridding_stats(which: str, k: int) -> dict:
    """``oracle.voxel_stats`` of field ``k``: what ``oracle.bound_ratio`` holds the weighted grid to."""
    d, masks = gridding(which), gridding_masks(which)
    mask = np.zeros(d["f0"].shape, bool) if masks[k] is None else masks[k]
    return oracle.voxel_stats(*gridding_neighbours(), d[f"f{k}"], mask)


def gridding_choice(which: str) -> np.ndarray:
    """int [3, nz, ny, nx]: the gate the closest-gate mode takes per field and voxel, -1 where it takes none."""
    s = cls.scene(GRIDDING_SCENE)
    return s.choice_for(gridding_masks(which), ("graph_replay", which))["idx32"][:GRIDDING_FIELDS]


SECTION_POINTS = 300
SECTION_ENDS = {"A": ((-9000.0, -3200.0), (9000.0, 3200.0)), "B": ((-8800.0, 3000.0), (9200.0, -2900.0))}      # (x, y) of both ends


@functools.lru_cache(maxsize=None)
def section_points(which: str):
    """``(xs, ys)`` float32 [SECTION_POINTS]: a straight path inside the lattice of the scene; B runs along the other diagonal.
    The points are device arrays of rg_roi_section_f32, not host-side parameters."""
    (x0, y0), (x1, y1) = SECTION_ENDS[which]
    xs, ys = np.linspace(x0, x1, SECTION_POINTS, dtype="float32"), np.linspace(y0, y1, SECTION_POINTS, dtype="float32")
    xs.setflags(write=False)
    ys.setflags(write=False)
    return xs, ys


@functools.lru_cache(maxsize=None)
def section_neighbours(which: str):
    s = cls.scene(GRIDDING_SCENE)
    zc = oracle.axis_coords_f32(s.limits[0][0], s.limits[0][1], s.shape[0])
    return ss.brute_section(s.gx, s.gy, s.gz, *section_points(which), zc, GRIDDING_WEIGHTING, exact_weights=True,
                            radar_altitude=s.radar_altitude, min_radius=s.min_radius, beam_factor=s.beam_factor, toa=s.toa)


def section_stats(which: str, k: int) -> dict:
    d, masks = gridding(which), gridding_masks(which)
    mask = np.zeros(d["f0"].shape, bool) if masks[k] is None else masks[k]
    return oracle.voxel_stats(*section_neighbours(which), d[f"f{k}"], mask)


def _gridding_expected(which):
    s, d, idx = cls.scene(GRIDDING_SCENE), gridding(which), gridding_choice(which)
    closest = np.stack([np.where(idx[k] >= 0, d[f"f{k}"][np.maximum(idx[k], 0)], np.float32(np.nan)) for k in range(GRIDDING_FIELDS)])
    weighted = np.stack([gridding_stats(which, k)["m"].astype(np.float32).reshape(s.shape) for k in range(GRIDDING_FIELDS)])
    section = np.stack([section_stats(which, k)["m"].astype(np.float32).reshape(s.shape[0], SECTION_POINTS) for k in range(GRIDDING_FIELDS)])
    return dict(closest=closest.astype(np.float32), weighted=weighted, section=section)


# ---- columns: slab_scenes' wide scene (6 x 10 x 150, 53 912 pairs, dense and wide chunks, a level without pairs), two fields ---------
# The CSR and its compact copy are geometry, built once outside every graph; the fields and their masks are the device data.
COLUMNS_WEIGHTING = "barnes2"
COLUMNS_FIELDS = 2
COLUMNS_PIECES = 2                # level pieces of the column and plane modes: the partial planes live in the workspace
COLUMNS_SEEDS = {"A": 61, "B": 67}


@functools.lru_cache(maxsize=None)
def columns(which: str) -> Dict[str, np.ndarray]:
    """``f0``, ``f1`` float32 [n_gates] and ``m0``, ``m1`` uint8 [n_gates] over the gates of the wide scene's volume."""
    n = int(sl.wide_scene()["vol"].gate_x.size)
    rng = np.random.default_rng(COLUMNS_SEEDS[which])
    out = {}
    for k in range(COLUMNS_FIELDS):
        out[f"f{k}"] = rng.normal(20.0, 10.0, n).astype(np.float32)
        out[f"m{k}"] = (rng.random(n) < 0.15).astype(np.uint8)
    return _frozen(out)


def columns_csr():
    """``(indptr, gate_indices, float32 weights)`` of the wide scene."""
    w = sl.wide_scene()
    return w["indptr"], w["idx"], w["w32"][COLUMNS_WEIGHTING]


@functools.lru_cache(maxsize=None)
def columns_grids(which: str):
    """``(row-wise order, tile order)`` float32 [F, nz, ny, nx]: the two restatements of the masked weighted mean, each with
    the float32 additions in the order its kernels document."""
    d = columns(which)
    fields, masks = [d[f"f{k}"] for k in range(COLUMNS_FIELDS)], [d[f"m{k}"] != 0 for k in range(COLUMNS_FIELDS)]
    shape = (COLUMNS_FIELDS,) + tuple(sl.WIDE_SHAPE)
    return (oracle.csr_apply_rowwise_order(*columns_csr(), fields, masks, sl.WIDE_SHAPE).reshape(shape),
            oracle.csr_apply_tile_order(*columns_csr(), fields, masks, sl.WIDE_SHAPE).reshape(shape))


def _columns_expected(which):
    rowwise, tile = columns_grids(which)
    nz = sl.WIDE_SHAPE[0]
    return dict(rowwise=rowwise, tile=tile,
                col_max=np.stack([oracle.column_max(g, 0, nz - 1) for g in rowwise]).astype(np.float32),
                col_arg=np.stack([oracle.column_argmax(g, 0, nz - 1) for g in rowwise]).astype(np.int32),
                col_min=np.stack([oracle.column_min(g, 0, nz - 1) for g in rowwise]).astype(np.float32))


# ---- mosaic: the mirror pair of combine_scenes' tie scene (3 x 9 x 21 voxels: eighteen workgroups), two fields, the tie path ----------
# The radars' gates, the per-radar searches and the path are geometry; the fields, their masks and the QC mask are device data.
MOSAIC_RADARS = cbs.TIE_MIRROR                   # table positions 0 and 1; on the column x = 0 their distances tie
MOSAIC_WEIGHTING = "barnes2"
MOSAIC_FIELDS = {"A": (0, 1), "B": (2, 3)}      # which fields of combine_scenes.field_set: B's are other moments, other masks
MOSAIC_COMBINE = "nearest_radar"


MOSAIC_THINNED = 0.6              # B: this share of the first radar's gates joins its QC mask, so the nearest radar changes


@functools.lru_cache(maxsize=None)
def _mosaic_field_set(which: str):
    """``combine_scenes.field_set`` of the tie scene; for B the QC mask of the first radar of the pair is thinned further."""
    fs, shared = cbs.field_set(cbs.tie_scene(), 4, masked=True)
    if which == "B":
        r = MOSAIC_RADARS[0]
        shared = list(shared)
        shared[r] = shared[r] | (np.random.default_rng(71).random(shared[r].size) < MOSAIC_THINNED)
    return fs, shared


@functools.lru_cache(maxsize=None)
def mosaic(which: str) -> Dict[str, np.ndarray]:
    """``f0``, ``f1`` float32 and ``m0``, ``m1``, ``shared`` uint8 over the gates of the two radars laid end to end."""
    fs, shared = _mosaic_field_set(which)
    out = {}
    for slot, k in enumerate(MOSAIC_FIELDS[which]):
        out[f"f{slot}"] = np.concatenate([fs[r][k][0] for r in MOSAIC_RADARS]).astype(np.float32)
        out[f"m{slot}"] = np.concatenate([fs[r][k][1] for r in MOSAIC_RADARS]).astype(np.uint8)
    out["shared"] = np.concatenate([shared[r] for r in MOSAIC_RADARS]).astype(np.uint8)
    return _frozen(out)


def mosaic_path():
    return cbs.path("tie")


def mosaic_stats(which: str, slot: int, section: bool, radar=None) -> dict:
    """``oracle.voxel_stats`` of field ``slot``: of the joint mean over both radars (``radar`` None), or of one radar alone
    (``radar``: its table position); on the lattice or at the samples of the path."""
    scene, (xs, ys) = cbs.tie_scene(), mosaic_path()
    fs, shared = _mosaic_field_set(which)
    k = MOSAIC_FIELDS[which][slot]
    if radar is None:
        d = mosaic(which)
        pairs = (mss.mosaic_csr(scene, MOSAIC_WEIGHTING, MOSAIC_RADARS, True, xs, ys, "graph_replay") if section
                 else scene.mosaic_csr(MOSAIC_WEIGHTING, MOSAIC_RADARS))
        return oracle.voxel_stats(*pairs, d[f"f{slot}"], (d[f"m{slot}"] != 0) | (d["shared"] != 0))
    r = MOSAIC_RADARS[radar]
    pairs = cbs.section_pairs(scene, MOSAIC_WEIGHTING, r, xs, ys, "graph_replay") if section else None
    return cbs.radar_stats(scene, MOSAIC_WEIGHTING, fs, shared, k, r, pairs)


def mosaic_nearest(which: str, slot: int, section: bool):
    """``(who uint8, m float64)``: the table position of the nearest radar that has a live neighbour (255: none has) by
    the rule of tests/test_gpu_mosaic_combine.py, and that radar's float64 mean."""
    scene, (xs, ys) = cbs.tie_scene(), mosaic_path()
    stats = [mosaic_stats(which, slot, section, radar) for radar in range(len(MOSAIC_RADARS))]
    d = np.stack([(cbs.section_d(scene, r, xs, ys) if section else cbs.lattice_d(scene, r)).ravel() for r in MOSAIC_RADARS])
    n = np.stack([s["n"] for s in stats])
    who = np.where((n > 0).any(axis=0), np.argmin(np.where(n > 0, d, np.inf), axis=0), cbs.NO_RADAR).astype(np.uint8)
    m = np.stack([s["m"] for s in stats] + [np.full(n.shape[1], np.nan)])
    return who, m[np.minimum(who, len(stats)), np.arange(n.shape[1])]


def _mosaic_expected(which):
    scene, n_points = cbs.tie_scene(), len(mosaic_path()[0])
    out = {}
    for section, shape in ((False, scene.shape), (True, (scene.shape[0], n_points))):
        tag = "section_" if section else ""
        out[tag + "mean"] = np.stack([mosaic_stats(which, s, section)["m"].astype(np.float32).reshape(shape) for s in (0, 1)])
        near = [mosaic_nearest(which, s, section) for s in (0, 1)]
        out[tag + "nearest"] = np.stack([m.astype(np.float32).reshape(shape) for _, m in near])
        out[tag + "radar"] = np.stack([who.reshape(shape) for who, _ in near])
    return out


# ---- prologue: the antenna transform on a small sweep table and two gate filters folded into one mask ---------------------------------
PROLOGUE_SWEEPS = (4, 30, 333)    # elevations, azimuths, gates: 39 960 gates
PROLOGUE_FILTERS = (("below", 10.0, 0.0), ("between", 30.0, 40.0))
PROLOGUE_MASK_BYTES = np.array([0, 1, 2, 0xFF], dtype=np.uint8)       # the prefilled bytes of tests/test_gpu_prologue.py


@functools.lru_cache(maxsize=None)
def prologue(which: str) -> Dict[str, np.ndarray]:
    """``ranges`` float64 [n_gates], ``az`` / ``el`` float64 [n_rays] (device tables of rg_antenna_to_cartesian_f32), ``data``
    float32 [n_rays * n_gates] and the ``mask`` uint8 the filters OR into.  B: another range table, every ray turned and
    lifted, other data and another mask."""
    from radar_processor_amd import synthetic
    n_elev, n_az, n_gates = PROLOGUE_SWEEPS
    elev, az, ranges = synthetic.sweep_geometry(n_elev, n_az, n_gates, max_range_m=120e3 if which == "A" else 97e3)
    if which == "B":
        elev, az = elev + 0.4, (az + 7.3) % 360.0
    rng = np.random.default_rng(81 if which == "A" else 83)
    n = n_elev * n_az * n_gates
    data = rng.normal(25.0, 15.0, n).astype(np.float32)
    data[rng.random(n) < 0.05] = np.nan
    return _frozen(dict(ranges=np.ascontiguousarray(ranges), az=np.tile(az, n_elev), el=np.repeat(elev, n_az), data=data,
                        mask=PROLOGUE_MASK_BYTES[rng.integers(4, size=n)]))


def _prologue_expected(which):
    d = prologue(which)
    x, y, z = oracle.antenna_to_cartesian(d["ranges"][None, :], d["az"][:, None], d["el"][:, None])
    shape = (d["az"].size, d["ranges"].size)
    mask = d["mask"].copy()
    for op, a, b in PROLOGUE_FILTERS:
        mask |= oracle.gate_mask(op, d["data"], np.float32(a), np.float32(b)).astype(np.uint8)
    out = {k: np.broadcast_to(v, shape).astype(np.float32).ravel() for k, v in (("x", x), ("y", y), ("z", z))}
    out["mask"] = mask
    return out


# ---- every chain ---------------------------------------------------------------------------------------------------------------------
_EXPECTED = dict(verification=_verification_expected, convection=_convection_expected, tracking=_tracking_expected,
                 raster=_raster_expected, accumulation=_accumulation_expected, motion=_motion_expected, cells=_cells_expected, products=_products_expected, georef=_georef_expected,
                 gridding=_gridding_expected, columns=_columns_expected, mosaic=_mosaic_expected, prologue=_prologue_expected)
# outputs the contract allows to be all zero or all fill: none of these chains has one
MAY_BE_TRIVIAL: Dict[str, Tuple[str, ...]] = {}
# outputs whose order the contract leaves open: compared as sets of rows
UNORDERED = {"tracking": ("pairs",)}
# outputs that follow from the host-side parameters alone (the lattice, the elevation): the same for A and B by construction;
# they are checked and poisoned like every other output, and the outputs computed from them differ
GEOMETRY_ONLY = {"products": ("sel", "w_hi", "level")}
# outputs with one row per cell: A and B differ in their number of rows
PER_CELL = {"cells": ("area", "bbox", "sum_yx", "vmax", "argmax", "vsum")}


@functools.lru_cache(maxsize=None)
def expected(chain: str, which: str) -> Dict[str, np.ndarray]:
    return _frozen({k: np.ascontiguousarray(v) for k, v in _EXPECTED[chain](which).items()})
