"""The generators and references of tests/product_scenes.py hold what tests/test_gpu_product_contracts.py relies on (no GPU
needed): the level-by-level column references agree with the oracle's NumPy reductions, every planted class is in every scene,
a contracted CAPPI blend would be seen, the restated PPI plan reproduces ``oracle.elevation_ppi`` and its exact pixels are
what they claim, and the raster references agree with matplotlib and NumPy."""
import numpy as np
import pytest

import product_scenes as ps
from oracle import radar_grid_oracle as oracle


def test_constants_are_the_build_s():
    from radar_processor_amd import _native
    assert ps.RG_PPI_SEL_NONE == _native.RG_PPI_SEL_NONE
    assert (ps.RG_TEST_LO, ps.RG_TEST_HI, ps.RG_TEST_LO_INCLUSIVE, ps.RG_TEST_NONFINITE) == \
        (_native.RG_TEST_LO, _native.RG_TEST_HI, _native.RG_TEST_LO_INCLUSIVE, _native.RG_TEST_NONFINITE)
    assert ps.N_CLASSES == 16 and len(set(ps.COLUMN_CLASSES)) == 16


# ---- column reduce ---------------------------------------------------------------------------------------------------------
def _equal_and_bits_off_zero(got, want, label):
    """assert_array_equal, and the same bits wherever the value is not a zero (NumPy's vectorised fmax / fmin loops do not
    promise which of +0.0 and -0.0 they keep; the level-by-level reference does)."""
    np.testing.assert_array_equal(got, want, err_msg=label)
    off_zero = ~(want == 0)
    assert ps.same_bits_or_both_nan(got, want)[off_zero].all(), label


@pytest.mark.parametrize("n_xy", ps.COLUMN_N_XY)
def test_column_references_agree_with_the_oracle_and_every_class_is_planted(n_xy):
    for s in ps.column_scenes(n_xy):
        label = f"nz {s.nz} n_xy {n_xy} window [{s.z_lo}, {s.z_hi}]"
        ref = ps.column_reduce_reference(s.grid, s.z_lo, s.z_hi)
        cube = s.grid.reshape(s.nz, 1, n_xy)
        _equal_and_bits_off_zero(ref.max, oracle.column_max(cube, s.z_lo, s.z_hi)[0], label + " max")
        _equal_and_bits_off_zero(ref.min, oracle.column_min(cube, s.z_lo, s.z_hi)[0], label + " min")
        np.testing.assert_array_equal(ref.argmax, oracle.column_argmax(cube, s.z_lo, s.z_hi)[0], err_msg=label + " argmax")
        sl = s.grid[s.z_lo:s.z_hi + 1]
        want_argmin = np.where(np.isnan(sl).all(axis=0), -1, np.argmin(np.where(np.isnan(sl), np.inf, sl), axis=0) + s.z_lo)
        np.testing.assert_array_equal(ref.argmin, want_argmin, err_msg=label + " argmin")
        assert ref.argmax.dtype == np.int32 and ref.argmin.dtype == np.int32 and ref.mean.dtype == np.float32
        # np.nanmean adds the levels in order only when it reduces over rows of more than one column: a single column is
        # one contiguous run, which NumPy sums pairwise (another float32 order from 8 levels on)
        if n_xy > 1:
            with np.errstate(all="ignore"):
                _equal_and_bits_off_zero(ref.mean, oracle.column_mean(cube, s.z_lo, s.z_hi)[0], label + " mean")
        # the planted classes
        w = s.z_hi - s.z_lo + 1
        for name, cols in s.classes.items():
            assert cols.size >= (1 if n_xy >= 16 else 0), f"{label}: class {name} is missing"
            for c in cols:
                assert ps.column_class_of(int(c), n_xy, s.seed)[0] == name
                assert ps.column_class_holds(s, name, int(c)), f"{label}: column {c} is no {name}"
        assert sum(c.size for c in s.classes.values()) == (min(n_xy, 16) if n_xy < 32 else
                                                           16 * (n_xy // 32) + min(n_xy % 32, 16))
        # what the classes are there for
        for c in s.classes["all_nan"]:
            assert np.isnan(ref.max[c]) and np.isnan(ref.min[c]) and np.isnan(ref.mean[c]) and ref.argmax[c] == ref.argmin[c] == -1
        for c in s.classes["last_only"]:
            assert ref.argmax[c] == ref.argmin[c] == s.z_hi and ps.bits(ref.max)[c] == ps.bits(s.grid[s.z_hi])[c]
        for c in s.classes["zeros_pos_first"]:
            assert ps.bits(ref.max)[c] == 0 and ps.bits(ref.min)[c] == 0 and ref.argmax[c] == ref.argmin[c] == s.z_lo
        for c in s.classes["zeros_neg_first"]:
            assert ps.bits(ref.max)[c] == 0x80000000 and ps.bits(ref.min)[c] == 0x80000000 and ref.argmax[c] == s.z_lo
        for c in s.classes["both_inf"]:
            assert np.isnan(ref.mean[c]) or w == 1
        for c in s.classes["flt_max"]:
            assert w < 2 or np.isinf(ref.mean[c])
        for name in ("tie_adjacent", "tie_stride4", "tie_first_last"):
            for c in s.classes[name]:
                first = ps._tie_levels(name, s.z_lo, s.z_hi)[0]
                assert (ref.argmin[c] if s.flipped[c] else ref.argmax[c]) == first
        if n_xy >= 64:        # ties for the maximum AND for the minimum
            tie_cols = np.concatenate([s.classes[k] for k in ("tie_adjacent", "tie_stride4", "tie_first_last")])
            assert s.flipped[tie_cols].any() and not s.flipped[tie_cols].all()


def test_small_scenes_rotate_through_every_class():
    """Below 16 columns a scene holds n_xy classes; the windows of one n_xy and the sizes 1, 3, 4 and 15 together hold all."""
    seen = {}
    for n_xy in (1, 3, 4, 15):
        for s in ps.column_scenes(n_xy):
            for name, cols in s.classes.items():
                if cols.size:
                    seen.setdefault(name, set()).add((n_xy, s.flipped[cols].any()))
    assert set(seen) == set(ps.COLUMN_CLASSES)
    for name in ("tie_adjacent", "tie_stride4", "tie_first_last"):
        assert {flip for _, flip in seen[name]} == {True, False}, name


def test_empty_window_reference():
    s = ps.column_scene(5, 20, 1)
    ref = ps.column_reduce_reference(s.grid, 3, 2)
    assert np.isnan(ref.max).all() and np.isnan(ref.min).all() and np.isnan(ref.mean).all()
    assert (ref.argmax == -1).all() and (ref.argmin == -1).all()


def test_level_outside_the_window_changes_the_result():
    """The levels around a window hold +-1e30 and NaN: a kernel reading one too many cannot pass."""
    s = ps.column_scene(13, 64, 3, z_lo=3, z_hi=10)
    inside = ps.column_reduce_reference(s.grid, 3, 10)
    for lo, hi in ((2, 10), (3, 11)):
        wider = ps.column_reduce_reference(s.grid, lo, hi)
        assert not ps.same_bits_or_both_nan(inside.max, wider.max).all() or not ps.same_bits_or_both_nan(inside.min, wider.min).all()
        assert not ps.same_bits_or_both_nan(inside.mean, wider.mean).all()


# ---- CAPPI blend -----------------------------------------------------------------------------------------------------------
def test_rounding_of_exact_values():
    from fractions import Fraction
    one = Fraction(1)
    assert ps._fraction_to_f32(one + Fraction(1, 2 ** 24)) == np.float32(1.0)                       # a tie: to even (down)
    assert ps._fraction_to_f32(one + Fraction(3, 2 ** 24)) == np.float32(1.0) + np.float32(2.0 ** -22)   # a tie: to even (up)
    assert ps._fraction_to_f32(one + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 80)) == np.nextafter(np.float32(1), np.float32(2))
    assert ps._fraction_to_f32(Fraction(1, 2 ** 149)) == np.float32(1e-45) and ps._fraction_to_f32(Fraction(0)) == 0


@pytest.mark.parametrize("weights", [(0.7, 0.3), (0.3, 0.7)])
def test_a_fused_blend_would_be_seen(weights):
    """For each contracted evaluation at least 5 % of the finite pixels of the 4096-pixel scene differ in bits from the
    contract's unfused float32 result (27 %, 20 % and 32 % with 0.7 / 0.3) -- and so do pixels of every scene of 255 pixels
    or more that the GPU test uses."""
    s = ps.lerp_scene(4096, 1, *weights)
    assert float(s.w_lo) not in (0.5, 0.25, 1.0) and s.w_lo.dtype == np.float32
    assert set(s.planted) == {"nan_lo", "nan_hi", "inf_times_w", "inf_minus_inf", "denormal_products", "denormal_inputs"}
    assert np.isnan(s.want[[s.planted[k] for k in ("nan_lo", "nan_hi", "inf_minus_inf")]]).all()
    assert s.want[s.planted["inf_times_w"]] == np.inf
    tiny = np.finfo(np.float32).tiny
    i = s.planted["denormal_products"]
    assert abs(s.lo[i]) >= tiny and 0 < abs(s.w_lo * s.lo[i]) < tiny and 0 < abs(s.w_hi * s.hi[i]) < tiny
    n_finite = int(s.finite.sum())
    assert n_finite >= 4090
    for name, alt in s.fused.items():
        share = float((ps.bits(alt) != ps.bits(s.want))[s.finite].mean())
        print(f"weights {weights}: {name} differs from the unfused blend on {100 * share:.1f} % of {n_finite} finite pixels")
        assert share >= 0.05, name
        assert np.abs(alt[s.finite].astype(np.float64) - s.want[s.finite]).max() <= 1e-5     # ... by a rounding, no more
    for n in ps.LERP_N_XY:
        small = ps.lerp_scene(n, n, *weights)
        if n >= 255:
            for name, alt in small.fused.items():
                assert int((ps.bits(alt) != ps.bits(small.want)).sum()) >= 10, (n, name)


def test_small_lerp_scenes_rotate_their_planted_pixels():
    seen = set()
    for seed in range(6):
        seen |= set(ps.lerp_scene(1, seed).planted) | set(ps.lerp_scene(5, seed).planted)
    assert len(seen) == 6


# ---- constant-elevation PPI ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [s.name for s in ps.ppi_scenes()])
def test_ppi_plan_combined_on_the_cpu(name):
    """Scenes derived from grid limits: the restated plan, combined on the CPU, is ``oracle.elevation_ppi`` bit for bit and
    the scalars are the Python layer's.  Every scene: the selection words unpack to levels of the grid."""
    s = ps.ppi_scene(name)
    for linear in (True, False):
        plan = ps.ppi_plan_reference(s, linear)
        got = ps.ppi_combine_reference(s.grid, plan, linear)
        assert got.dtype == (np.float64 if linear else np.float32) and got.shape == (s.ny, s.nx)
        sel = plan.sel[plan.in_range]
        assert ((sel & 0xFFFF) < s.nz).all() and ((sel >> 16) < s.nz).all() and (sel >= 0).all()
        assert (plan.sel[~plan.in_range] == ps.RG_PPI_SEL_NONE).all()
        if linear:
            assert ((plan.w_hi >= 0) & (plan.w_hi < 1))[plan.in_range].all()
        else:
            assert ((sel & 0xFFFF) == (sel >> 16)).all()
        if s.oracle_args is not None:
            limits, elev, curved = s.oracle_args
            with np.errstate(all="ignore"):
                want = oracle.elevation_ppi(s.grid, limits, elev, "linear" if linear else "nearest", earth_curvature=curved)
            assert ps.same_bits_or_both_nan(got, want).all(), f"{name} linear {linear}"
            assert plan.in_range.any() and (name.endswith("one_level") or not plan.in_range.all())
    assert (s.oracle_args is not None) == name.startswith("from_limits")


def test_ppi_exact_pixels():
    s = ps.ppi_scene("flat_exact")
    lin, near = ps.ppi_plan_reference(s, True), ps.ppi_plan_reference(s, False)
    m = s.marks
    assert lin.tz[m["half_2"]] == 2500.0 and lin.tz[m["half_4"]] == 3500.0 and lin.tz[m["top"]] == 5000.0
    assert lin.zf[m["half_2"]] == 2.5 and lin.zf[m["half_4"]] == 3.5 and lin.zf[m["half_4_mirror"]] == 3.5
    assert near.lo_s[m["half_2"]] == 2 and near.lo_s[m["half_4"]] == 4 and near.lo_s[m["half_4_mirror"]] == 4   # half to even
    assert near.sel[m["half_2"]] == 2 | 2 << 16 and near.sel[m["half_4"]] == 4 | 4 << 16
    assert lin.sel[m["half_2"]] == 2 | 3 << 16 and lin.w_hi[m["half_2"]] == 0.5
    # the origin sits on z_min, (6000, 8000) on z_max: both in range, the upper level clamped
    assert lin.tz[m["origin"]] == 0.0 == s.z_min and lin.in_range[m["origin"]] and lin.sel[m["origin"]] == 0 | 1 << 16
    assert lin.in_range[m["top"]] and lin.sel[m["top"]] == 5 | 5 << 16 and lin.w_hi[m["top"]] == 0.0
    # z_max one float64 below / above 5000
    below, above = ps.ppi_scene("flat_exact_zmax_below"), ps.ppi_scene("flat_exact_zmax_above")
    assert below.z_max < 5000.0 < above.z_max
    assert not ps.ppi_plan_reference(below, True).in_range[m["top"]] and ps.ppi_plan_reference(above, True).in_range[m["top"]]
    assert ps.ppi_plan_reference(below, False).in_range[m["top"]]                       # nearest: level 5 either way
    # z_min on 2500 and on its neighbours
    on, lo, hi = (ps.ppi_scene("flat_exact_zmin" + k) for k in ("", "_below", "_above"))
    assert lo.z_min < on.z_min == 2500.0 < hi.z_min
    p_on, p_lo, p_hi = (ps.ppi_plan_reference(x, True) for x in (on, lo, hi))
    assert p_on.in_range[m["half_2"]] and p_on.zf[m["half_2"]] == 0.0 and p_lo.in_range[m["half_2"]]
    assert not p_hi.in_range[m["half_2"]] and p_hi.zf[m["half_2"]] < 0 and p_hi.lo_s[m["half_2"]] == 0
    assert ps.ppi_plan_reference(hi, False).sel[m["half_2"]] == 0                       # nearest: rint(-tiny) is level 0
    assert not p_on.in_range[m["origin"]]
    # a negative elevation: the same half-way pixels below the radar
    neg = ps.ppi_plan_reference(ps.ppi_scene("flat_negative"), False)
    assert neg.tz[m["half_2"]] == -2500.0 and neg.zf[m["half_2"]] == 2.5 and neg.lo_s[m["half_2"]] == 2
    # one level
    one = ps.ppi_scene("one_level")
    assert one.nz == 1 and one.z_step == 1.0
    p = ps.ppi_plan_reference(one, True)
    assert p.in_range[one.marks["on_level"]] and p.sel[one.marks["on_level"]] == 0 and int(p.in_range.sum()) == 1
    q = ps.ppi_plan_reference(one, False)
    assert q.in_range[one.marks["on_level"]] and 1 <= int(q.in_range.sum()) < q.in_range.size
    # the curved scene holds its origin pixel
    curved = ps.ppi_scene("from_limits_curved")
    assert curved.curved == 1 and curved.xc[8] == 0.0 and curved.yc[6] == 0.0


def test_collapse_ppi_reference_is_the_oracle_s():
    rng = np.random.default_rng(2)
    grid = rng.normal(0, 10, (5, 6, 7)).astype(np.float32)
    x, y, z = np.linspace(-50e3, 50e3, 7), np.linspace(-40e3, 40e3, 6), np.linspace(0, 4000.0, 5)
    for elev in (0.5, 3.0):
        plane, level = ps.collapse_ppi_reference(grid, x, y, z, float(np.sin(np.deg2rad(elev))), 2.0 * oracle.PROCESSOR_EARTH_RADIUS)
        np.testing.assert_array_equal(level, oracle.ppi_levels(x, y, z, elev))
        np.testing.assert_array_equal(plane, np.asarray(oracle.collapse_3d_to_2d(grid, "ppi", x, y, z, elevation_deg=elev)))
    z_nan = np.array([0.0, np.nan, 2000.0, np.nan, 4000.0])
    assert (ps.collapse_ppi_reference(grid, x, y, z_nan, 0.05, 1.7e7)[1] == 1).all()


# ---- raster ----------------------------------------------------------------------------------------------------------------
def _plane(dtype, seed=4, n=3000):
    rng = np.random.default_rng(seed)
    data = rng.normal(15.0, 20.0, n).astype(dtype)
    data[rng.random(n) < 0.2] = np.nan
    data[rng.random(n) < 0.1] = -9999.0
    return data


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("fill", [None, -9999.0])
def test_colormap_reference_is_matplotlib_s(dtype, fill):
    from radar_processor_amd.raster import colormap_lut
    data = _plane(dtype).reshape(50, 60)
    data[0, :4] = [-5.0, 45.5, 45.5 - 1e-3, 1e30]                  # vmin, vmax and their neighbourhood
    for cmap in ("viridis", "tab10"):
        lut = colormap_lut(cmap)
        for vmin, vmax in ((-5.0, 45.5), (7.0, 7.0), (0.0, 1e-3)):
            want = oracle.colormap_rgba(data, cmap, vmin, vmax, fill_value=fill)
            got = ps.colormap_reference(data, vmin, vmax, lut, fill=fill)
            np.testing.assert_array_equal(got, want, err_msg=f"{cmap} [{vmin}, {vmax}] fill {fill}")


def test_colormap_reference_on_explicit_tables():
    lut = ps.random_lut(7, 1)
    assert len({tuple(r) for r in lut.tolist()}) == 10 and (lut[:, 3] > 0).all()
    data = np.array([0.0, 7.0, 6.999, 3.5, -1.0, 9.0, np.nan, -9999.0], dtype=np.float32)
    got = ps.colormap_reference(data, 0.0, 7.0, lut)
    assert got[:, :3].tolist() == lut[[0, 6, 6, 3, 0, 6, 9, 0], :3].tolist()          # v == n_lut -> the last entry; NaN -> bad
    assert got[:, 3].tolist() == lut[[0, 6, 6, 3, 0, 6], 3].tolist() + [0, lut[0, 3]]
    got = ps.colormap_reference(data, 0.0, 7.0, lut, fill=-9999.0)
    assert got[6].tolist() == lut[9].tolist() and got[7].tolist() == lut[0, :3].tolist() + [0]   # a NaN is data next to a fill
    assert (ps.colormap_reference(data, 2.0, 2.0, lut)[:, :3] == lut[0, :3]).all()
    one = ps.random_lut(1, 2)
    assert (ps.colormap_reference(data[:6], 0.0, 7.0, one) == one[0]).all()
    assert ps.random_lut(4093, 3).shape == (4096, 4)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_minmax_reference_is_geotiff_s(dtype):
    """radar_grid/geotiff.py:111-125: valid_data = data[~nodata]; np.nanmin / np.nanmax / len(valid_data)."""
    data = _plane(dtype)
    for fill in (None, -9999.0):
        nodata = np.isnan(data) if fill is None else data == fill
        valid = data[~nodata]
        got = ps.minmax_reference(data, fill)
        assert got.dtype == np.float64
        assert got[0] == np.nanmin(valid) and got[1] == np.nanmax(valid) and got[3] == len(valid)
        assert got[2] == np.count_nonzero(~np.isnan(valid)) and (fill is None) == (got[2] == got[3])
    assert ps.minmax_reference(np.zeros(0, dtype=dtype)).tolist() == [np.inf, -np.inf, 0.0, 0.0]
    assert ps.minmax_reference(np.full(5, np.nan, dtype=dtype), -9999.0).tolist() == [np.inf, -np.inf, 0.0, 5.0]
    # the fill value is compared in the data's dtype
    odd = np.array([-9999.9, 1.0], dtype=dtype)
    assert ps.minmax_reference(odd, -9999.9)[3] == 1.0
    if dtype == np.float32:
        assert ps.minmax_reference(odd.astype(np.float64), -9999.9)[3] == 2.0


def test_filter_references_are_numpy_s():
    rng = np.random.default_rng(6)
    src = rng.normal(15.0, 20.0, 500).astype(np.float32)
    src[::7] = np.nan
    src[3], src[4] = np.inf, -np.inf
    thr = 15.000001                                                # float32 does not hold it
    src[5], src[6] = np.float32(thr), np.nextafter(np.float32(thr), np.float32(0))
    masked, out = ps.plane_filter_reference(src, None, [(None, thr, 40.3, ps.RG_TEST_LO | ps.RG_TEST_HI)])
    with np.errstate(invalid="ignore"):
        want = np.isnan(src) | (src < thr) | (src > 40.3)          # a float32 array against Python floats: float32 comparisons
    np.testing.assert_array_equal(masked, want)
    assert not masked[5] and masked[6] and masked[4] and masked[3]
    assert ps.plane_filter_reference(src, None, [(None, thr, 0.0, ps.RG_TEST_LO | ps.RG_TEST_LO_INCLUSIVE)])[0][5]
    assert (ps.bits(out)[~masked] == ps.bits(src)[~masked]).all() and np.isnan(out[masked]).all()
    mask = ps.MASK_BYTES[rng.integers(5, size=500)]
    masked, _ = ps.plane_filter_reference(src, mask, [])
    np.testing.assert_array_equal(masked, mask != 0)               # an explicit mask is authoritative: a NaN is not masked
    # GridFilter: copy, boolean mask, assignment (radar_grid/filters.py:655-779)
    for dtype in (np.float32, np.float64):
        plane = src.astype(dtype)
        want = plane.copy()
        with np.errstate(invalid="ignore"):
            want[(want < thr) | (want > 40.3)] = -9999.0
        got = ps.grid_filter_reference(plane, ps.RG_TEST_LO | ps.RG_TEST_HI, thr, 40.3, None, -9999.0)
        np.testing.assert_array_equal(got, want)
        assert got.dtype == dtype and np.isnan(got[::7]).all()
        got = ps.grid_filter_reference(plane, ps.RG_TEST_NONFINITE, 0.0, 0.0, mask, np.nan)
        np.testing.assert_array_equal(np.isnan(got), ~np.isfinite(plane) | (mask != 0))
