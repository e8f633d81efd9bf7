"""Plain NumPy / Python restatements and hand-made inputs for the kernels behind the gridders: ``rg_column_reduce_f32``,
``rg_cappi_lerp_f32``, ``rg_elevation_ppi_f32`` and its plan / finish halves (csrc/rg_products.hip), ``rg_collapse_ppi_f32``,
``rg_plane_filter_f32``, ``rg_grid_filter``, ``rg_nan_minmax`` and ``rg_colormap_rgba`` (csrc/rg_raster.hip) -- written from
the contracts in include/radargrid_hip.h, never from the kernels.  Everything here is selection, integer work or IEEE
arithmetic in a stated order, so every reference is meant to be compared bit for bit.  No GPU is needed: what the generators
promise is asserted by tests/test_product_scenes.py, what the kernels do with them by tests/test_gpu_product_contracts.py."""
import functools
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

F32 = np.float32
INF32 = F32(np.inf)
FLT_MAX = np.finfo(np.float32).max
RG_PPI_SEL_NONE = -1
RG_TEST_LO, RG_TEST_HI, RG_TEST_LO_INCLUSIVE, RG_TEST_NONFINITE = 1, 2, 4, 8
MASK_BYTES = np.array([0, 1, 2, 0x80, 0xFF], dtype=np.uint8)


def bits(a) -> np.ndarray:
    """The bit patterns of a float32 (uint32) or float64 (uint64) array."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits_or_both_nan(got, want) -> np.ndarray:
    """bool per element: equal bit patterns, or a NaN on both sides (a NaN's payload is nobody's contract)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


# ---- column reduce ---------------------------------------------------------------------------------------------------------
def column_reduce_reference(grid, z_lo: int, z_hi: int) -> SimpleNamespace:
    """``grid`` float32 ``[nz, n_xy]`` -> max / argmax / min / argmin / mean over levels ``z_lo .. z_hi``, level by level:

    * max and min start from the first non-NaN level and then keep the accumulator when ``acc >= v`` (max) / ``acc <= v``
      (min) or when ``v`` is NaN -- so the first of equal values wins, the sign of a zero included;
    * the arg is the level that supplied the kept value, ``-1`` for an all-NaN column;
    * the mean adds float32 values in level order, from float32 0.0, a NaN counting as 0.0, and is
      ``(float32)(float64(sum) / count)``: NaN where the count is 0.

    An empty window (``z_lo > z_hi``) is all-NaN / ``-1``."""
    grid = np.asarray(grid)
    assert grid.dtype == np.float32 and grid.ndim == 2
    n = grid.shape[1]
    out = {}
    with np.errstate(all="ignore"):
        for name, is_max in (("max", True), ("min", False)):
            acc = np.full(n, np.nan, dtype=np.float32)
            arg = np.full(n, -1, dtype=np.int32)
            for z in range(z_lo, z_hi + 1):
                v = grid[z]
                unseen = arg < 0
                keep = ((acc >= v) if is_max else (acc <= v)) | np.isnan(v)
                take = np.where(unseen, ~np.isnan(v), ~keep)
                acc = np.where(take, v, acc)
                arg = np.where(take, np.int32(z), arg)
            out[name], out["arg" + name] = acc, arg
        total = np.zeros(n, dtype=np.float32)
        count = np.zeros(n, dtype=np.int64)
        for z in range(z_lo, z_hi + 1):
            v = grid[z]
            nan = np.isnan(v)
            total = total + np.where(nan, F32(0.0), v)               # float32 + float32: one float32 rounding per level
            count += ~nan
        assert total.dtype == np.float32
        out["mean"] = (total.astype(np.float64) / count.astype(np.float64)).astype(np.float32)
    return SimpleNamespace(**out)


COLUMN_CLASSES = ("all_nan", "nan_first", "last_only", "quarter_0", "quarter_1", "quarter_2", "quarter_3", "tie_adjacent",
                  "tie_stride4", "tie_first_last", "pos_inf", "neg_inf", "both_inf", "zeros_pos_first", "zeros_neg_first",
                  "flt_max")
N_CLASSES = len(COLUMN_CLASSES)            # 16: one full cycle fits every n_xy >= 16
CYCLE = 2 * N_CLASSES                      # 16 planted columns, then 16 random ones
TIE = F32(75.5)                            # outside the random values' range (-50, 50): the planted levels are the extremum


def column_class_of(c: int, n_xy: int, seed: int):
    """(class name or None for a random column, flipped?) of column ``c``.  Columns come in cycles of 32: the 16 planted
    classes, then 16 random columns, so that every ``n_xy >= 16`` holds each class; below 16 the classes rotate with the
    seed.  A flipped column is negated (a maximum tie becomes a minimum tie); the flip alternates per cycle and with the
    seed, and never touches the classes that are named after a sign."""
    if n_xy < N_CLASSES:
        slot = (c + seed) % N_CLASSES
    else:
        slot = c % CYCLE
        if slot >= N_CLASSES:
            return None, bool((c // CYCLE + seed + 1) % 2)
    name = COLUMN_CLASSES[slot]
    flip = bool((c // CYCLE + seed) % 2) and name.startswith(("tie_", "quarter_", "last_only", "flt_max"))
    return name, flip


def _tie_levels(name, z_lo, z_hi):
    w = z_hi - z_lo + 1
    if name == "tie_adjacent":            # neighbours: two different level quarters -- the partial results' tie rule
        a = z_lo + (1 if w >= 3 else 0)
        return a, min(a + 1, z_hi)
    if name == "tie_stride4":             # four apart: the same level quarter -- the accumulator's tie rule
        a = z_lo + (1 if w >= 6 else 0)
        return a, min(a + 4, z_hi)
    return z_lo, z_hi                     # tie_first_last


def column_scene(nz: int, n_xy: int, seed: int, z_lo: int = 0, z_hi: int = None) -> SimpleNamespace:
    """A float32 grid ``[nz, n_xy]`` of random columns (normal(10, 15), a quarter of the levels NaN) and planted ones, the
    planted cases placed relative to the level window ``z_lo .. z_hi`` (default: all levels):

    ``all_nan``; ``nan_first`` -- NaN at the window's first level, DENORMALS of both signs above it; ``last_only`` -- a value
    at the last level only; ``quarter_q`` -- non-NaN exactly at the levels with ``(z - z_lo) % 4 == q`` (the level quarter
    one lane group of the split kernel covers; ``z % 4 == q`` for a window starting at 0; all NaN when the window has no
    such level); ``tie_adjacent`` / ``tie_stride4`` / ``tie_first_last`` -- the extremum at two levels ``z, z + 1`` /
    ``z, z + 4`` / first and last; ``pos_inf`` / ``neg_inf`` / ``both_inf`` (the mean of the last is NaN);
    ``zeros_pos_first`` / ``zeros_neg_first`` -- nothing but zeros of alternating sign, ``+0.0`` resp. ``-0.0`` first;
    ``flt_max`` -- ``FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX`` repeating: the float32 running sum overflows where a wider
    one would come back to 0.

    Levels outside the window hold +-1e30 and NaN: reading one of them changes every result.  ``classes`` maps a class
    name to its columns, ``flipped`` marks negated columns (see :func:`column_class_of`)."""
    z_hi = nz - 1 if z_hi is None else z_hi
    assert 0 <= z_lo <= z_hi < nz
    rng = np.random.default_rng([seed, nz, n_xy, z_lo, z_hi])
    w = z_hi - z_lo + 1
    grid = rng.normal(10.0, 15.0, (nz, n_xy)).astype(np.float32)
    grid[rng.random((nz, n_xy)) < 0.25] = np.nan
    outside = np.where(rng.random((nz, n_xy)) < 0.3, np.nan, np.where(rng.random((nz, n_xy)) < 0.5, 1e30, -1e30)).astype(np.float32)
    classes = {k: [] for k in COLUMN_CLASSES}
    flipped = np.zeros(n_xy, dtype=bool)
    rel = np.arange(w)
    for c in range(n_xy):
        name, flip = column_class_of(c, n_xy, seed)
        flipped[c] = flip
        if name is None:
            col = grid[z_lo:z_hi + 1, c].copy()
        else:
            classes[name].append(c)
            col = np.full(w, np.nan, dtype=np.float32)
            if name == "nan_first":
                tiny = rng.integers(1, 0x007FFFFF, size=w).astype(np.uint32) | (rng.integers(0, 2, size=w).astype(np.uint32) << 31)
                col[:] = tiny.view(np.float32)
                col[0] = np.nan
            elif name == "last_only":
                col[-1] = F32(rng.normal(10.0, 15.0))
            elif name.startswith("quarter_"):
                q = int(name[-1])
                col[rel % 4 == q] = rng.normal(10.0, 15.0, int((rel % 4 == q).sum())).astype(np.float32)
            elif name.startswith("tie_"):
                col[:] = rng.uniform(-50.0, 50.0, w).astype(np.float32)
                a, b = _tie_levels(name, z_lo, z_hi)
                col[a - z_lo] = col[b - z_lo] = TIE
            elif name.endswith("_inf"):
                col[:] = rng.normal(10.0, 15.0, w).astype(np.float32)
                if name in ("pos_inf", "both_inf"):
                    col[w // 2] = np.inf
                if name == "neg_inf":
                    col[w // 3] = -np.inf
                if name == "both_inf":
                    col[(w // 2 + 1) % w] = -np.inf          # a one-level window keeps -inf alone
            elif name.startswith("zeros_"):
                first_negative = name == "zeros_neg_first"
                col[:] = np.where((rel % 2 == 1) != first_negative, F32(-0.0), F32(0.0))
            elif name == "flt_max":
                col[:] = np.where(rel % 4 < 2, FLT_MAX, -FLT_MAX)
        if flip:
            col = -col
        grid[z_lo:z_hi + 1, c] = col
    grid[:z_lo] = outside[:z_lo]
    grid[z_hi + 1:] = outside[z_hi + 1:]
    return SimpleNamespace(grid=np.ascontiguousarray(grid), nz=nz, n_xy=n_xy, z_lo=z_lo, z_hi=z_hi, seed=seed,
                           classes={k: np.array(v, dtype=np.int64) for k, v in classes.items()}, flipped=flipped)


# What tests/test_gpu_product_contracts.py runs rg_column_reduce_f32 on: (nz, z_lo, z_hi).  nz = 7: the sequential kernel; a
# window of 8 levels or more: the level range split over four lane groups -- lengths 8, 9, 11 and 13, starting at 0, 1 and 3;
# one level.
COLUMN_N_XY = (1, 3, 4, 15, 16, 17, 60, 64, 68, 1023, 1024, 1028, 4100)
COLUMN_WINDOWS = ((7, 0, 6), (8, 0, 7), (8, 1, 6), (11, 0, 10), (11, 1, 9), (11, 3, 10), (13, 0, 12), (13, 1, 11), (13, 3, 10),
                  (13, 5, 5))
LERP_N_XY = (1, 5, 255, 256, 260, 1028)


def column_scenes(n_xy: int):
    """The scenes of one ``n_xy``, one per window of COLUMN_WINDOWS; the seed moves with both, so that below 16 columns
    the classes rotate and the flipped columns alternate."""
    return [column_scene(nz, n_xy, seed=n_xy + i, z_lo=lo, z_hi=hi) for i, (nz, lo, hi) in enumerate(COLUMN_WINDOWS)]


def column_class_holds(s, name: str, c: int) -> bool:
    """Does column ``c`` of scene ``s`` have the property class ``name`` stands for?  (What test_product_scenes.py asserts
    of every planted column, stated on the data alone.)"""
    col = s.grid[s.z_lo:s.z_hi + 1, c]
    w = col.size
    ok = ~np.isnan(col)
    rel = np.arange(w)
    if name == "all_nan":
        return not ok.any()
    if name == "nan_first":
        return bool(np.isnan(col[0])) and (w == 1 or bool((np.abs(col[1:]) < np.finfo(np.float32).tiny).all() and (col[1:] != 0).all()))
    if name == "last_only":
        return bool(ok[-1]) and not ok[:-1].any()
    if name.startswith("quarter_"):
        return bool((ok == (rel % 4 == int(name[-1]))).all())
    if name.startswith("tie_"):
        a, b = (z - s.z_lo for z in _tie_levels(name, s.z_lo, s.z_hi))
        top = np.nanmin(col) if s.flipped[c] else np.nanmax(col)
        hits = np.nonzero(col == top)[0]
        return abs(float(top)) == float(TIE) and hits.tolist() == sorted({a, b})
    if name == "pos_inf":
        return bool((col == np.inf).any()) and not (col == -np.inf).any()
    if name == "neg_inf":
        return bool((col == -np.inf).any()) and not (col == np.inf).any()
    if name == "both_inf":
        return bool((col == -np.inf).any()) and (w == 1 or bool((col == np.inf).any()))
    if name.startswith("zeros_"):
        sign = np.signbit(col)
        return bool((col == 0).all()) and bool(sign[0]) == (name == "zeros_neg_first") and bool((sign[1:] != sign[:-1]).all())
    if name == "flt_max":
        return bool((np.abs(col) == FLT_MAX).all()) and (w < 2 or col[0] == col[1])
    raise KeyError(name)


# ---- CAPPI blend -----------------------------------------------------------------------------------------------------------
def _fraction_to_f32(x: Fraction) -> np.float32:
    """The float32 nearest to the rational ``x`` (ties to even): ONE rounding of an exact value."""
    if x == 0:
        return F32(0.0)
    near = F32(float(x))                                    # within one float32 step of the answer
    best = None
    for cand in (near, np.nextafter(near, INF32), np.nextafter(near, -INF32)):
        if not np.isfinite(cand):
            continue
        err = abs(Fraction(float(cand)) - x)
        even = (int(np.array([cand]).view(np.uint32)[0]) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even):
            best = (err, cand)
    return best[1]


@functools.lru_cache(maxsize=None)
def lerp_scene(n: int, seed: int, w_lo: float = 0.7, w_hi: float = 0.3) -> SimpleNamespace:
    """Two float32 levels ``lo`` / ``hi`` of ``n`` normal(10, 15) pixels and the float32 weights (0.7 and 0.3: neither is a
    power of two, so both products round), with planted pixels -- NaN in either level, ``inf * w``, ``inf - inf``, products
    in the denormal range -- at the front when ``n >= 8``, rotating with the seed below that.

    ``want`` is the contract: ``fl32(fl32(w_lo * lo) + fl32(w_hi * hi))``.  ``fused`` holds what three contracted evaluations
    would give instead: ``fma_first = fl32(w_lo * lo + fl32(w_hi * hi))``, ``fma_second = fl32(fl32(w_lo * lo) + w_hi * hi)``
    and ``exact = fl32(w_lo * lo + w_hi * hi)`` -- the unrounded terms carried exactly (rational arithmetic), one rounding.
    ``finite`` marks the pixels whose inputs and results are all finite."""
    rng = np.random.default_rng([seed, n])
    lo = rng.normal(10.0, 15.0, n).astype(np.float32)
    hi = rng.normal(10.0, 15.0, n).astype(np.float32)
    planted = [("nan_lo", np.nan, 3.0), ("nan_hi", 3.0, np.nan), ("inf_times_w", np.inf, 3.0), ("inf_minus_inf", np.inf, -np.inf),
               ("denormal_products", 1.5e-38, -1.3e-38), ("denormal_inputs", 3.0e-42, 5.0e-44)]
    where = {}
    for k, (name, a, b) in enumerate(planted):
        if n >= 8:
            i = k
        elif (k + seed) % len(planted) < n:
            i = (k + seed) % len(planted)
        else:
            continue
        lo[i], hi[i] = a, b
        where[name] = i
    wl, wh = F32(w_lo), F32(w_hi)
    with np.errstate(all="ignore"):
        p_lo, p_hi = wl * lo, wh * hi
        assert p_lo.dtype == np.float32 and p_hi.dtype == np.float32
        want = p_lo + p_hi
    finite = np.isfinite(lo) & np.isfinite(hi) & np.isfinite(want)
    fused = {k: want.copy() for k in ("fma_first", "fma_second", "exact")}
    fl, fh = Fraction(float(wl)), Fraction(float(wh))
    for i in np.nonzero(finite)[0]:
        e_lo, e_hi = fl * Fraction(float(lo[i])), fh * Fraction(float(hi[i]))
        fused["fma_first"][i] = _fraction_to_f32(e_lo + Fraction(float(p_hi[i])))
        fused["fma_second"][i] = _fraction_to_f32(Fraction(float(p_lo[i])) + e_hi)
        fused["exact"][i] = _fraction_to_f32(e_lo + e_hi)
    for a in (lo, hi, want, finite, *fused.values()):
        a.setflags(write=False)
    return SimpleNamespace(n=n, lo=lo, hi=hi, w_lo=wl, w_hi=wh, want=want, fused=fused, finite=finite, planted=where)


# ---- constant-elevation PPI ------------------------------------------------------------------------------------------------
def ppi_plan_reference(s, linear: bool) -> SimpleNamespace:
    """The per-pixel plan of a constant-elevation PPI from the scalars the C ABI takes (``s``: a :func:`ppi_scenes` entry):
    float32 ground range ``sqrt(x*x + y*y)``; float64 target altitude, 4/3-earth
    ``sqrt((sr*sr + ke_re_sq) + ((2*sr)*ke_re)*sin_elev) - ke_re`` with ``sr = range / cos_clamped`` or flat ``range *
    tan_elev``; ``zf = (tz - z_min) / z_step``.  Linear: ``lo = floor(zf)``, ``w_hi = zf - lo``, levels ``lo`` and ``lo + 1``
    clamped to the grid, no value where ``tz < z_min`` or ``tz > z_max``.  Nearest: ``k = rint(zf)`` (half to even), no value
    where ``k`` is outside the grid.  ``sel = lo | hi << 16`` or ``RG_PPI_SEL_NONE``."""
    yy, xx = np.meshgrid(s.yc, s.xc, indexing="ij")
    assert xx.dtype == np.float32
    hd = np.sqrt(xx * xx + yy * yy)
    assert hd.dtype == np.float32
    if s.curved:
        sr = hd.astype(np.float64) / s.cos_c
        tz = np.sqrt((sr * sr + s.ke_re2) + ((2.0 * sr) * s.ke_re) * s.sin_e) - s.ke_re + 0.0
    else:
        tz = hd.astype(np.float64) * s.tan_e + 0.0
    zf = (tz - s.z_min) / s.z_step
    if linear:
        lo = np.floor(zf).astype(np.int64)
        w_hi = zf - lo
        lo_s, hi_s = np.clip(lo, 0, s.nz - 1), np.clip(lo + 1, 0, s.nz - 1)
        in_range = ~((tz < s.z_min) | (tz > s.z_max))
    else:
        k = np.round(zf).astype(np.int64)
        w_hi = np.zeros_like(zf)
        lo_s = hi_s = np.clip(k, 0, s.nz - 1)
        in_range = (k >= 0) & (k < s.nz)
    sel = np.where(in_range, lo_s | (hi_s << 16), RG_PPI_SEL_NONE).astype(np.int32)
    return SimpleNamespace(tz=tz, zf=zf, lo_s=lo_s, hi_s=hi_s, w_hi=w_hi, in_range=in_range, sel=sel)


def ppi_combine_reference(grid, plan, linear: bool) -> np.ndarray:
    """The plan applied to a stored grid ``[nz, ny, nx]`` on the CPU: float64 ``(1 - w_hi) * v_lo + w_hi * v_hi`` (linear)
    or the float32 value of the nearest level, NaN where the pixel has no value."""
    iy, ix = np.meshgrid(np.arange(grid.shape[1]), np.arange(grid.shape[2]), indexing="ij")
    v_lo, v_hi = grid[plan.lo_s, iy, ix], grid[plan.hi_s, iy, ix]
    with np.errstate(all="ignore"):
        if linear:
            out = (1.0 - plan.w_hi) * v_lo.astype(np.float64) + plan.w_hi * v_hi.astype(np.float64)
        else:
            out = v_lo.copy()
    out[~plan.in_range] = np.nan
    return out


def _ppi_scene(name, xc, yc, nz, scalars, seed, oracle_args=None, marks=None):
    cos_c, sin_e, tan_e, ke_re, ke_re2, z_min, z_max, z_step, curved = scalars
    xc, yc = np.ascontiguousarray(xc, dtype=np.float32), np.ascontiguousarray(yc, dtype=np.float32)
    rng = np.random.default_rng([seed, nz, xc.size, yc.size])
    grid = rng.normal(10.0, 15.0, (nz, yc.size, xc.size)).astype(np.float32)
    grid[rng.random(grid.shape) < 0.15] = np.nan
    grid[rng.random(grid.shape) < 0.03] = np.inf
    grid[rng.random(grid.shape) < 0.03] = -np.inf
    return SimpleNamespace(name=name, xc=xc, yc=yc, nz=int(nz), ny=int(yc.size), nx=int(xc.size), grid=grid, cos_c=float(cos_c),
                           sin_e=float(sin_e), tan_e=float(tan_e), ke_re=float(ke_re), ke_re2=float(ke_re2), z_min=float(z_min),
                           z_max=float(z_max), z_step=float(z_step), curved=int(curved), oracle_args=oracle_args,
                           marks=marks or {})


def ppi_scalars(s, linear: bool) -> tuple:
    """The scalar arguments of ``rg_elevation_ppi_f32`` / ``_plan_f32`` after the shape, in ABI order."""
    return (s.cos_c, s.sin_e, s.tan_e, s.ke_re, s.ke_re2, s.z_min, s.z_max, s.z_step, s.curved, int(linear))


def _from_limits(name, shape, limits, elevation_deg, curved, seed):
    """A scene whose tables and scalars are what the Python layer derives from a geometry (``_ppi_scalars``): the one kind
    ``oracle.elevation_ppi`` can be asked about."""
    from radar_processor_amd.grid_products import EFFECTIVE_RADIUS_FACTOR, _ppi_scalars
    geometry = SimpleNamespace(grid_shape=shape, grid_limits=limits)
    (nz, _, _), xc, yc, sc = _ppi_scalars(geometry, elevation_deg, "linear", curved, EFFECTIVE_RADIUS_FACTOR)
    return _ppi_scene(name, xc, yc, nz, sc[:9], seed, oracle_args=(limits, elevation_deg, bool(curved)))


@functools.lru_cache(maxsize=None)
def ppi_scenes() -> tuple:
    """The PPI scenes, by name.

    ``flat_exact*``: flat earth, ``tan_elev = 0.5``, ``z_step = 1000``, six levels, tables holding (3000, 4000), (4200, 5600)
    and (6000, 8000): ground ranges exactly 5000, 7000 and 10000, target altitudes 2500, 3500 and 5000.  With
    ``z_min = 0`` the first two sit at ``zf`` = 2.5 and 3.5 -- nearest levels 2 and 4 by round half to even -- and the
    third ON ``z_max = 5000``; ``_zmax_below`` / ``_zmax_above`` move ``z_max`` to the float64 neighbours of 5000 (the pixel
    leaves / stays in the linear range); ``flat_exact_zmin*`` put ``z_min`` on 2500 and on its two neighbours.  The origin is
    a pixel of every one of them.  ``flat_negative``: ``tan_elev = -0.5`` over levels -5000 .. 0.  ``one_level``: ``nz = 1``,
    ``z_step = 1.0``.  ``from_limits_*``: tables and scalars as the Python layer derives them from grid limits (flat, curved,
    a negative angle, one level) -- the scenes ``oracle.elevation_ppi`` is compared on.  ``marks`` names planted pixels as
    ``(iy, ix)``."""
    xc = [-4200.0, 0.0, 3000.0, 4200.0, 6000.0, 6500.0]
    yc = [0.0, 4000.0, 5600.0, 8000.0, -5600.0]
    marks = dict(half_2=(1, 2), half_4=(2, 3), top=(3, 4), origin=(0, 1), half_4_mirror=(4, 0))
    flat = lambda z_min, z_max, tan=0.5: (1.0, 0.0, tan, 8494666.0, 8494666.0 ** 2, z_min, z_max, 1000.0, 0)
    up, down = (lambda v: float(np.nextafter(v, np.inf))), (lambda v: float(np.nextafter(v, -np.inf)))
    scenes = [
        _ppi_scene("flat_exact", xc, yc, 6, flat(0.0, 5000.0), 1, marks=marks),
        _ppi_scene("flat_exact_zmax_below", xc, yc, 6, flat(0.0, down(5000.0)), 2, marks=marks),
        _ppi_scene("flat_exact_zmax_above", xc, yc, 6, flat(0.0, up(5000.0)), 3, marks=marks),
        _ppi_scene("flat_exact_zmin", xc, yc, 6, flat(2500.0, 7500.0), 4, marks=marks),
        _ppi_scene("flat_exact_zmin_below", xc, yc, 6, flat(down(2500.0), 7500.0), 5, marks=marks),
        _ppi_scene("flat_exact_zmin_above", xc, yc, 6, flat(up(2500.0), 7500.0), 6, marks=marks),
        _ppi_scene("flat_negative", xc, yc, 6, flat(-5000.0, 0.0, tan=-0.5), 7, marks=marks),
        _ppi_scene("one_level", [0.0, 3000.0, 5001.0, 5002.0, 3000.5], [0.0, 4000.0], 1, flat(2500.0, 2500.0)[:7] + (1.0, 0), 8,
                   marks=dict(on_level=(1, 1), origin=(0, 0))),
        _from_limits("from_limits_flat", (9, 13, 17), ((0.0, 8000.0), (-100e3, 100e3), (-120e3, 120e3)), 4.0, False, 9),
        _from_limits("from_limits_curved", (16, 13, 17), ((0.0, 3000.0), (-100e3, 100e3), (-120e3, 120e3)), 2.0, True, 10),
        _from_limits("from_limits_curved_steep", (7, 5, 259), ((500.0, 9500.0), (-30e3, 30e3), (-40e3, 40e3)), 19.5, True, 11),
        _from_limits("from_limits_negative", (6, 9, 11), ((-1500.0, 1000.0), (-50e3, 50e3), (-50e3, 50e3)), -2.0, True, 12),
        _from_limits("from_limits_one_level", (1, 7, 9), ((0.0, 0.0), (-10.0, 10.0), (-10.0, 10.0)), 3.0, False, 13),
    ]
    return tuple(scenes)


def ppi_scene(name: str) -> SimpleNamespace:
    return next(s for s in ppi_scenes() if s.name == name)


# ---- processor-style PPI collapse ------------------------------------------------------------------------------------------
def collapse_ppi_reference(grid, x, y, z, sin_elev: float, two_re: float):
    """``(plane float32 [ny, nx], level int32 [ny, nx])``: float64 ``r = sqrt(x^2 + y^2)``, ``zt = r * sin_elev + r^2 /
    two_re``, level = ``np.argmin(|zt - z|)`` -- the first minimum, a NaN counting as the minimum (so the first NaN entry of
    ``z`` wins every pixel) --, plane = ``grid[level]``."""
    xs, ys = np.meshgrid(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), indexing="xy")
    r = np.sqrt(xs * xs + ys * ys)
    zt = r * sin_elev + (r * r) / two_re
    level = np.argmin(np.abs(zt[..., None] - np.asarray(z, dtype=np.float64)[None, None, :]), axis=2).astype(np.int32)
    iy, ix = np.meshgrid(np.arange(len(y)), np.arange(len(x)), indexing="ij")
    return grid[level, iy, ix], level


# ---- min / max / counts ----------------------------------------------------------------------------------------------------
def minmax_reference(data, fill=None) -> np.ndarray:
    """float64 ``[min, max, number of non-NaN valid pixels, number of valid pixels]``: a pixel is no-data when it equals
    ``fill`` -- compared in the data's dtype -- or, without a fill value, when it is NaN; min and max ignore NaN and are
    +inf / -inf when nothing is left."""
    data = np.asarray(data).ravel()
    assert data.dtype in (np.float32, np.float64)
    nodata = np.isnan(data) if fill is None else data == data.dtype.type(fill)
    valid = data[~nodata]
    numbers = valid[~np.isnan(valid)]
    lo = float(numbers.min()) if numbers.size else np.inf
    hi = float(numbers.max()) if numbers.size else -np.inf
    return np.array([lo, hi, float(numbers.size), float(valid.size)], dtype=np.float64)


# ---- plane filter ----------------------------------------------------------------------------------------------------------
def plane_filter_reference(src, src_mask, tests):
    """``(masked bool, out float32)`` of ``rg_plane_filter_f32``.  ``tests``: ``(plane or None, lo, hi, flags)``; a test drops
    a pixel when the tested value ``q`` (the plane's, or the source's) is ``< lo`` (RG_TEST_LO), ``<= lo`` (with
    RG_TEST_LO_INCLUSIVE as well), ``> hi`` (RG_TEST_HI) or not finite (RG_TEST_NONFINITE), thresholds rounded to float32; a
    pixel is already masked when ``src_mask`` is non-zero there or, without one, when the source is NaN.  ``out`` holds
    NaN where masked and the source's own bits elsewhere."""
    src = np.asarray(src)
    assert src.dtype == np.float32
    drop = np.zeros(src.shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        for plane, lo, hi, flags in tests:
            q = src if plane is None else np.asarray(plane)
            assert q.dtype == np.float32
            if flags & RG_TEST_LO:
                drop |= (q <= F32(lo)) if flags & RG_TEST_LO_INCLUSIVE else (q < F32(lo))
            if flags & RG_TEST_HI:
                drop |= q > F32(hi)
            if flags & RG_TEST_NONFINITE:
                drop |= ~np.isfinite(q)
    masked = drop | ((np.asarray(src_mask) != 0) if src_mask is not None else np.isnan(src))
    return masked, np.where(masked, F32(np.nan), src)


# ---- grid filter -----------------------------------------------------------------------------------------------------------
def grid_filter_reference(src, flags: int, lo: float, hi: float, mask, fill_value: float) -> np.ndarray:
    """``out = hit ? fill_value : src`` with ``hit = v < lo`` (RG_TEST_LO) ``or v > hi`` (RG_TEST_HI) ``or v`` not finite
    (RG_TEST_NONFINITE) ``or mask != 0``; thresholds and fill value rounded to the plane's dtype first."""
    src = np.asarray(src)
    t = src.dtype.type
    assert t in (np.float32, np.float64)
    hit = np.zeros(src.shape, dtype=bool) if mask is None else np.asarray(mask) != 0
    with np.errstate(invalid="ignore"):
        if flags & RG_TEST_LO:
            hit = hit | (src < t(lo))
        if flags & RG_TEST_HI:
            hit = hit | (src > t(hi))
        if flags & RG_TEST_NONFINITE:
            hit = hit | ~np.isfinite(src)
    return np.where(hit, t(fill_value), src)


# ---- colormap --------------------------------------------------------------------------------------------------------------
def colormap_reference(data, vmin: float, vmax: float, lut, fill=None) -> np.ndarray:
    """uint8 ``data.shape + (4,)``.  ``lut``: uint8 ``[n_lut + 3, 4]`` -- the table, then the under, over and bad colours.
    In float64 whatever the data's dtype: ``v = minimum(maximum(x, vmin), vmax)`` (NaN propagates), ``v -= vmin``,
    ``v /= vmax - vmin``, ``v *= n_lut``, ``v == n_lut -> n_lut - 1``; index ``trunc(v)``, ``n_lut`` when ``v < 0``,
    ``n_lut + 1`` when ``v >= n_lut``, ``n_lut + 2`` when NaN; ``vmin == vmax`` selects entry 0 everywhere.  Alpha is 0 where
    the pixel is no-data: equal to ``fill`` in the data's dtype or, without a fill value, NaN."""
    data = np.asarray(data)
    lut = np.asarray(lut)
    assert data.dtype in (np.float32, np.float64) and lut.dtype == np.uint8 and lut.ndim == 2 and lut.shape[1] == 4
    n_lut = lut.shape[0] - 3
    assert n_lut >= 1 and not vmin > vmax
    nodata = np.isnan(data) if fill is None else data == data.dtype.type(fill)
    if vmin == vmax:
        idx = np.zeros(data.shape, dtype=np.int64)
    else:
        with np.errstate(all="ignore"):
            v = np.minimum(np.maximum(data.astype(np.float64), np.float64(vmin)), np.float64(vmax))
            v = v - np.float64(vmin)
            v = v / (np.float64(vmax) - np.float64(vmin))
            v = v * np.float64(n_lut)
            v = np.where(v == n_lut, np.float64(n_lut - 1), v)
            idx = np.where(np.isnan(v), n_lut + 2, np.where(v < 0, n_lut, np.where(v >= n_lut, n_lut + 1,
                                                                                 np.trunc(np.nan_to_num(v)).astype(np.int64))))
    rgba = lut[idx].copy()
    rgba[nodata, 3] = 0
    return rgba


def random_lut(n_lut: int, seed: int) -> np.ndarray:
    """uint8 ``[n_lut + 3, 4]`` with every row different from every other (so a wrong index is a wrong colour) and no
    alpha of 0 (so a cleared alpha is seen)."""
    rng = np.random.default_rng([seed, n_lut])
    rows = rng.choice(1 << 24, size=n_lut + 3, replace=False).astype(np.uint32)
    lut = np.empty((n_lut + 3, 4), dtype=np.uint8)
    lut[:, 0], lut[:, 1], lut[:, 2] = rows & 0xFF, (rows >> 8) & 0xFF, (rows >> 16) & 0xFF
    lut[:, 3] = rng.integers(1, 256, size=n_lut + 3)
    return lut
