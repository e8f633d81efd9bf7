"""Scenes for the nowcast kernels (csrc/rg_motion.hip, rg_accumulate.hip, rg_verify.hip, rg_convection.hip) at the sizes where
a LAUNCH-GEOMETRY constant is exceeded -- what the scene files of the four families, which stop at 700 x 600 pixels, 24 layers,
six planes and three pairs, never reach:

``layer_split``   5000 planes of 3 x 5 under 8 thresholds: 40 000 layers, so ``rg_fss_sums_i32`` takes a second launch whose
                  ``layer0`` is not 0;
``layer_limit``   as many planes of 1 x 3 as ``gridDim.y`` holds, one threshold: the contingency grid and the column grid of the
                  table at their limit, the sums in two launches;
``four_trips``    one plane of 3 1/8 x ``kMaxStrips`` x ``kBlock`` pixels: every workgroup of the contingency and of the sums
                  kernel walks three full trips of its grid-stride loop, the first eighth of them a fourth;
``tall`` / ``wide``   70 003 x 3 and 3 x 70 001: thousands of trips of the column pass (with an unroll remainder) and of the row
                  pass (with a cut last trip and a carry beyond 2^16);
``plane_limit``   as many planes of 2 x 3 as ``gridDim.y`` holds through all four convection stages;
``wrap_row``      one row of 3 000 000 pixels, uniform 85 dBZ and drawn from 60 .. 80 dBZ: on the uniform row the 64-bit prefix
                  of q passes 2^63 and then 2^64 inside the row -- "exact modulo 2^64" put to work;
``group_split``   4 x 65535, 4 x 65535 + 3 and 4 x 65537 + 2 planes of 2 x 3 through the accumulation: the limit of one launch
                  with and without a remainder, and two groups beyond it;
``many_pairs``    4099 plane pairs of 12 x 20 through the block match (``blockIdx.x / (nby * nbx)``) and 4099 planes through the
                  advection's plane loop.

Every launch constant is READ from the kernel sources, so a changed constant moves the shape or fails
tests/test_nowcast_scale_scenes.py.  The stacks with a period hold plane ``p % 61``: 61 is prime and divides neither 4 nor
65535 nor 32768 nor any launch offset made of them, so a plane read or written at a wrong launch offset meets another plane.
Everything is deterministic, computed once, read-only, and importable without a GPU."""
import functools
import os
import re

import numpy as np

import accumulation_oracle as ao
import accumulation_scenes as acs
import convection_oracle as co
import convection_scenes as cvs
import motion_oracle as mo
import verification_oracle as vo
import verification_scenes as vs

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "radar_processor_amd", "csrc")


@functools.lru_cache(maxsize=None)
def _source(source):
    with open(os.path.join(_CSRC, source)) as f:
        return f.read()


def _constant(source, name):
    """``<name> = <integer>`` inside a ``constexpr int`` statement of a kernel source, or None when it is not there."""
    found = re.search(r"^\s*constexpr\s+int\s+[^;]*\b%s\s*=\s*(\d+)\s*[,;]" % name, _source(source), flags=re.M)
    return int(found.group(1)) if found else None


def _cap(source, what):
    """The integer of ``RG_REQUIRE(<what> <= <integer>,`` of a kernel source, or None."""
    found = re.search(r"RG_REQUIRE\(\s*%s\s*<=\s*(\d+)\s*," % what, _source(source))
    return int(found.group(1)) if found else None


BLOCK = _constant("rg_common.hpp", "kBlock")                    # threads of a workgroup
WAVE = _constant("rg_common.hpp", "kWave")                      # pixels of one trip of a row pass
MAX_STRIPS = _constant("rg_verify.hip", "kMaxStrips")           # gridDim.x cap of the contingency and the sums kernel
LAYERS_PER_LAUNCH = _constant("rg_verify.hip", "kLayersPerLaunch")
COLUMN_UNROLL = _constant("rg_verify.hip", "kColumnUnroll")
CONTINGENCY_MAX_PLANES = _cap("rg_verify.hip", "n_planes")      # gridDim.y of contingency_kernel
SAT_MAX_LAYERS = _cap("rg_verify.hip", "layers")                # gridDim.y of sat_columns_kernel
CONVECTION_MAX_PLANES = _constant("rg_convection.hip", "kMaxPlanes")      # gridDim.y of the background and the area kernel
PLANES = _constant("rg_accumulate.hip", "kPlanes")              # planes of one group of the accumulation
MAX_GROUPS = _constant("rg_accumulate.hip", "kMaxGroups")       # gridDim.y of one accumulation launch
TILE_W, TILE_H = _constant("rg_accumulate.hip", "kTileW"), _constant("rg_accumulate.hip", "kTileH")
CONSTANTS = dict(kBlock=BLOCK, kWave=WAVE, kMaxStrips=MAX_STRIPS, kLayersPerLaunch=LAYERS_PER_LAUNCH, kColumnUnroll=COLUMN_UNROLL,
                 contingency_planes=CONTINGENCY_MAX_PLANES, sat_layers=SAT_MAX_LAYERS, kMaxPlanes=CONVECTION_MAX_PLANES,
                 kPlanes=PLANES, kMaxGroups=MAX_GROUPS, kTileW=TILE_W, kTileH=TILE_H)
_FOUND = all(v is not None for v in CONSTANTS.values())

PERIOD = 61


# ---- what a shape reaches: the launch arithmetic of the host code, restated -------------------------------------------------------
def strips(hw):
    """Workgroups along x of ``contingency_kernel`` / ``fss_sums_kernel`` for a plane of ``hw`` pixels."""
    return min(-(-hw // BLOCK), MAX_STRIPS)


def strip_trips(hw):
    """``(full, cut)``: the trips EVERY workgroup makes through its grid-stride loop, and how many workgroups make one more."""
    step = strips(hw) * BLOCK
    return hw // step, -(-(hw % step) // BLOCK)


def fss_launches(n_layers):
    """The layer counts of the launches of ``rg_fss_sums_i32``; launch ``k`` starts at layer ``k * kLayersPerLaunch``."""
    return [min(n_layers - first, LAYERS_PER_LAUNCH) for first in range(0, n_layers, LAYERS_PER_LAUNCH)]


def row_trips(w):
    """``(trips, pixels of the last one)`` of a row pass over ``w`` pixels."""
    return -(-w // WAVE), w - (-(-w // WAVE) - 1) * WAVE


def accumulation_runs(n_planes):
    """``(groups of every launch of full groups, planes of the remainder launch)`` of ``rg_accumulate_advected_f32``."""
    groups = n_planes // PLANES
    return [min(groups - first, MAX_GROUPS) for first in range(0, groups, MAX_GROUPS)], n_planes % PLANES


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


# ---- verification --------------------------------------------------------------------------------------------------------------
SPLIT_PLANES, SPLIT_SHAPE = 5000, (3, 5)
SPLIT_LEVELS = (-5.0, 3.0, 12.0, 21.0, 30.0, 40.0, 48.0, 55.0, 60.0)      # one level between any two of ROWS_THRESHOLDS
FOUR_TRIPS_SHAPE = ((MAX_STRIPS, (3 * MAX_STRIPS + MAX_STRIPS // 8) * BLOCK // MAX_STRIPS) if _FOUND else None)      # 1024 x 800
TALL_SHAPE = (8750 * COLUMN_UNROLL + 3, 3) if _FOUND else None                                                       # 70 003 x 3
WIDE_SHAPE = (3, 1093 * WAVE + 49) if _FOUND else None                                                               # 3 x 70 001
VERIFICATION = ("layer_split", "layer_limit", "four_trips", "tall", "wide")


def _mostly_exceeding(shape, seed):
    """Levels around 18 and 35 of which 98 % reach 18: a row of 70 001 carries more than 2^16 exceedances; 1 % NaN."""
    rng = np.random.default_rng(seed)
    out = np.asarray((5.0, 20.0, 36.0, 50.0), np.float32)[rng.choice(4, shape, p=(0.01, 0.5, 0.3, 0.19))]
    out[rng.random(shape) < 0.01] = np.nan
    return out


def _mask(shape, seed, share):
    rng = np.random.default_rng(seed)
    return (rng.random(shape) < share).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)


def _build_verification(name):
    if name == "layer_split":
        shape = (SPLIT_PLANES,) + SPLIT_SHAPE
        return vs.Scene(name, vs.levels(shape, 31, SPLIT_LEVELS, 0.04), vs.levels(shape, 32, SPLIT_LEVELS, 0.04), _mask(shape, 33, 0.03),
                        vs.ROWS_THRESHOLDS, (1, 2, 3, 255))
    if name == "layer_limit":
        shape = (CONTINGENCY_MAX_PLANES, 1, 3)
        return vs.Scene(name, vs.levels(shape, 34, (5.0, 18.0, 35.0), 0.1), vs.levels(shape, 35, (5.0, 18.0, 35.0), 0.1), None, (18.0,),
                        (1, 2, 255))
    if name == "four_trips":
        shape = (1,) + FOUR_TRIPS_SHAPE
        rng = np.random.default_rng(36)
        forecast = rng.uniform(0.0, 60.0, shape).astype(np.float32)
        observed = np.where(rng.random(shape) < 0.7, forecast, rng.uniform(0.0, 60.0, shape)).astype(np.float32)
        forecast[rng.random(shape) < 0.01] = np.nan
        observed[rng.random(shape) < 0.01] = np.nan
        mask = np.zeros(shape, dtype=np.uint8)
        mask[:, 900:940, 100:700] = 1                       # in the fourth trip's pixels too: they start at row 960
        mask[:, 1000:1010, 300:420] = 9
        return vs.Scene(name, forecast, observed, mask, (10.0, 40.0), (1, 16, 255))
    if name in ("tall", "wide"):
        shape = (1,) + (TALL_SHAPE if name == "tall" else WIDE_SHAPE)
        seed = 37 if name == "tall" else 39
        return vs.Scene(name, _mostly_exceeding(shape, seed), _mostly_exceeding(shape, seed + 1), None, (18.0, 35.0), (1, 255))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def verification_scene(name) -> vs.Scene:
    s = _build_verification(name)
    _frozen(s.forecast, s.observed, s.mask)
    return s


@functools.lru_cache(maxsize=None)
def verification_expected(name) -> vs.Expected:
    """The restated result of a verification scene (``verification_oracle``), as ``verification_scenes.expected`` forms it."""
    s = verification_scene(name)
    c = vo.contingency(s.forecast, s.observed, s.thresholds, s.mask)
    out = vs.Expected(c.counts, c.valid, vo.sat(s.forecast, s.thresholds, s.observed, s.mask),
                      vo.sat(s.observed, s.thresholds, s.forecast, s.mask),
                      vo.fss_sums(s.forecast, s.observed, s.thresholds, s.scales, s.mask))
    _frozen(*out)
    return out


# ---- convection ----------------------------------------------------------------------------------------------------------------
PLANE_LIMIT_SHAPE = (2, 3)
WRAP_WIDTH = 3_000_000
WRAP_DBZ = 85.0                                             # clamps to 80: q = 65536 * 10^8 on every pixel
WRAP_Q = 65536 * 10 ** 8
WRAP_ROWS = ("wrap_row_uniform", "wrap_row_drawn")


def _build_convection(name):
    hw, fps = cvs._disks()
    if name == "plane_limit":
        shape = (CONVECTION_MAX_PLANES,) + PLANE_LIMIT_SHAPE
        rng = np.random.default_rng(41)
        dbz = rng.uniform(0.0, 60.0, shape).astype(np.float32)
        dbz[rng.random(shape) < 0.08] = np.nan
        return cvs.Scene(name, dbz, _mask(shape, 42, 0.05), hw, fps, cvs.EDGES)
    if name == "wrap_row_uniform":
        return cvs.Scene(name, np.full((1, 1, WRAP_WIDTH), WRAP_DBZ, np.float32), None, hw, fps, cvs.EDGES)
    if name == "wrap_row_drawn":
        rng = np.random.default_rng(43)
        dbz = rng.uniform(60.0, 80.0, (1, 1, WRAP_WIDTH)).astype(np.float32)
        dbz[rng.random(dbz.shape) < 0.02] = np.nan
        return cvs.Scene(name, dbz, None, hw, fps, cvs.EDGES)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def convection_scene(name) -> cvs.Scene:
    s = _build_convection(name)
    _frozen(s.dbz, s.mask)
    return s


@functools.lru_cache(maxsize=None)
def plane_limit_expected() -> cvs.Expected:
    """The whole chain of ``convection_oracle`` on ``plane_limit`` with NumPy's own q, as ``convection_scenes.expected``."""
    s = convection_scene("plane_limit")
    q, e = co.quantize(s.dbz, s.mask, s.min_dbz), co.echo(s.dbz, s.mask, s.min_dbz)
    S, N, bkg = co.background(s.dbz, s.hw, s.mask, s.min_dbz, q)
    c = co.centres(s.dbz, bkg, s.edges, s.mask, s.min_dbz, s.intense, s.peak)
    out = cvs.Expected(q, e, S, N, bkg, c, co.area(c, s.dbz, s.footprints, s.mask, s.min_dbz))
    _frozen(*out)
    return out


def wrap_background(name, q=None):
    """``(q, S, N, bkg)`` of a ``wrap_row`` scene by ``convection_oracle.background``, whose int64 prefix wraps where the
    device's unsigned one does; ``q`` replaces NumPy's own quantisation (the device's, in the GPU test)."""
    s = convection_scene(name)
    q = co.quantize(s.dbz, s.mask, s.min_dbz) if q is None else q
    out = (q,) + co.background(s.dbz, s.hw, s.mask, s.min_dbz, q)
    _frozen(*out)
    return out


@functools.lru_cache(maxsize=None)
def wrap_expected(name):
    """:func:`wrap_background` with NumPy's q, computed once."""
    return wrap_background(name)


def wrap_window(width=None):
    """int64 ``[w]``: the pixels of the background window of a one-row plane that lie in the row -- ``N`` of the uniform row."""
    width = WRAP_WIDTH if width is None else width
    half = int(cvs._disks()[0][0])
    x = np.arange(width, dtype=np.int64)
    return np.minimum(x + half, width - 1) - np.maximum(x - half, 0) + 1


def wrap_column(q=None):
    """The first column of a ``wrap_row`` scene whose inclusive prefix of ``q`` is 2^64 or more, from Python integers; None
    when the row's total stays below it.  ``q`` None: the uniform row."""
    if q is None:
        column = -(-2 ** 64 // WRAP_Q) - 1
        return column if column < WRAP_WIDTH else None
    total = 0
    for column, v in enumerate(np.asarray(q).ravel().tolist()):
        total += v
        if total >= 2 ** 64:
            return column
    return None


# ---- accumulation --------------------------------------------------------------------------------------------------------------
GROUP_SPLIT_SHAPE = (2, 3)
GROUP_SPLIT_PLANES = ((PLANES * MAX_GROUPS, PLANES * MAX_GROUPS + 3, PLANES * (MAX_GROUPS + 2) + 2) if _FOUND else ())
GROUP_SPLIT_METHODS = ("nearest", "bilinear")
GROUP_SPLIT_VECTOR = (0.75, -0.5)


def _group_split_rates(seed):
    """``accumulation_scenes.rates`` with holes.  It puts two +inf pixels into every plane, which on six pixels would leave
    little but +inf in the results: all but every eighth plane get a finite rate there instead, its own."""
    base = acs.rates(GROUP_SPLIT_SHAPE, PERIOD, seed, True)
    for k in range(PERIOD):
        if k % 8:
            base[k][np.isinf(base[k])] = np.float32(100.0 + 0.5 * k)
    return base


@functools.lru_cache(maxsize=None)
def group_split_scene(method) -> acs.Scene:
    """The PERIOD base planes of ``group_split`` as one call; plane ``p`` of a stack of any height holds plane ``p % PERIOD``."""
    motion, lat = acs.one_node(GROUP_SPLIT_VECTOR)
    s = acs.Scene("group_split_" + method, _group_split_rates(51), _group_split_rates(52), motion, lat, 0.25, 3, 2, method, 2, acs.FILL,
                  True)
    _frozen(s.prev, s.next, s.motion)
    return s


@functools.lru_cache(maxsize=None)
def group_split_expected(method) -> ao.Accumulation:
    """``accumulation_oracle.accumulate`` on the PERIOD base planes: the planes are independent, so plane ``p`` of the stack
    has the result of plane ``p % PERIOD``."""
    s = group_split_scene(method)
    want = ao.accumulate(s.prev, s.next, s.motion, s.lattice, s.hours, s.n_steps, s.substeps, s.method, s.min_steps, s.fill)
    _frozen(want.out, want.steps)
    return want


# ---- motion --------------------------------------------------------------------------------------------------------------------
MANY_PAIRS = 4099
PAIR_SHAPE = (12, 20)
PAIR_B, PAIR_S, PAIR_R = 8, 4, 2
PAIR_QUIET = (7, 30, 52)                                    # base pairs whose western blocks hold no echo
ADVECT_LEADS = (1.0, 2.5)
ADVECT_SUBSTEPS = 2
ADVECT_FILL = -9.25
ADVECT_METHODS = ("nearest", "bilinear")


@functools.lru_cache(maxsize=None)
def many_pairs_levels():
    """``(prev, next)`` uint8 ``[PERIOD, 12, 20]``: random levels, a quarter of them 0 (no echo); ``next`` is ``prev`` moved by
    a displacement within the search radius that changes from pair to pair, with a tenth of its pixels drawn again."""
    rng = np.random.default_rng(61)
    shape = (PERIOD,) + PAIR_SHAPE
    prev = rng.integers(1, 256, shape).astype(np.uint8)
    prev[rng.random(shape) < 0.25] = 0
    for k in PAIR_QUIET:
        prev[k][:, :12] = 0
    nxt = np.empty_like(prev)
    for k in range(PERIOD):
        nxt[k] = np.roll(prev[k], (k % 5 - 2, k // 5 % 5 - 2), axis=(0, 1))
    again = rng.random(shape) < 0.1
    nxt[again] = rng.integers(0, 256, shape).astype(np.uint8)[again]
    _frozen(prev, nxt)
    return prev, nxt


@functools.lru_cache(maxsize=None)
def many_pairs_match() -> mo.Match:
    """``motion_oracle.block_match`` of the PERIOD base pairs; pair ``p`` of the stack has the result of pair ``p % PERIOD``."""
    m = mo.block_match(*many_pairs_levels(), PAIR_B, PAIR_S, PAIR_R)
    _frozen(*m)
    return m


@functools.lru_cache(maxsize=None)
def advect_base():
    """``(planes float32 [PERIOD, 12, 20] with NaN and +inf, motion float32 [2, 4, 2], lattice)``: the block lattice of the
    match above with fractional vectors."""
    planes = acs.rates(PAIR_SHAPE, PERIOD, 62, True)
    lat = mo.block_lattice(PAIR_SHAPE, PAIR_B, PAIR_S)
    motion = acs.fractional(lat, 63, 3.0)
    _frozen(planes, motion)
    return planes, motion, lat


@functools.lru_cache(maxsize=None)
def advect_expected(method):
    """``motion_oracle.advect`` of the PERIOD base planes: float32 ``[leads, PERIOD, 12, 20]``."""
    planes, motion, lat = advect_base()
    out = mo.advect(planes, motion, lat, ADVECT_LEADS, ADVECT_SUBSTEPS, method, ADVECT_FILL)
    _frozen(out)
    return out


def periodic(base, count):
    """``base[p % PERIOD]`` for ``p`` in ``0 .. count - 1`` along the first axis."""
    return np.ascontiguousarray(base[np.arange(count) % PERIOD])


def distinct(planes):
    """Whether no two entries along the first axis hold the same bytes."""
    return len({np.ascontiguousarray(p).tobytes() for p in planes}) == len(planes)
