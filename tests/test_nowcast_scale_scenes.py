"""CPU-side checks of tests/nowcast_scale_scenes.py (no GPU needed): each scene reaches the launch path it was built for, with
the numbers derived from the constants READ from the kernel sources -- a second launch with ``layer0 != 0``, three full trips
and a cut fourth of a grid-stride loop, ``gridDim.y`` at its limit, a 64-bit prefix that wraps inside the row, full groups
beyond one launch -- so a changed kernel constant fails here, loudly, and does not silently shrink what
tests/test_gpu_nowcast_scale.py covers.  And every entry point that puts a plane or layer count into ``gridDim.y`` refuses one
more than it holds, on the host, before it touches a device."""
import ctypes
import time

import numpy as np
import pytest

import accumulation_scenes as acs
import convection_oracle as co
import nowcast_scale_scenes as ns
import verification_oracle as vo


def test_the_whole_module_builds_in_a_few_seconds():
    """Every scene and every restated result: what the GPU file pays before its launches.  First in the file, so that the
    caches are cold when the whole file runs; a guard against a scene that became slow, not a measurement."""
    start = time.perf_counter()
    for name in ns.VERIFICATION:
        ns.verification_expected(name)
    ns.plane_limit_expected()
    for name in ns.WRAP_ROWS:
        ns.wrap_expected(name)
    for method in ns.GROUP_SPLIT_METHODS:
        ns.group_split_expected(method)
    ns.many_pairs_match()
    for method in ns.ADVECT_METHODS:
        ns.advect_expected(method)
    total = time.perf_counter() - start
    print(f"all scenes with every restated result: {total:.2f} s")
    assert total < 15.0


def test_launch_constants_were_found_in_the_sources():
    missing = [name for name, value in ns.CONSTANTS.items() if value is None]
    assert not missing, f"not found in the kernel sources: {missing}"
    assert ns.BLOCK % ns.WAVE == 0 and ns.TILE_W * ns.TILE_H == ns.BLOCK
    # every plane or layer count that goes into gridDim.y is capped at the same number
    assert ns.CONTINGENCY_MAX_PLANES == ns.SAT_MAX_LAYERS == ns.CONVECTION_MAX_PLANES == ns.MAX_GROUPS
    # the shapes the module's docstring states, with the constants as they are today
    if (ns.BLOCK, ns.WAVE, ns.MAX_STRIPS, ns.LAYERS_PER_LAUNCH, ns.COLUMN_UNROLL, ns.PLANES, ns.MAX_GROUPS) == (256, 64, 1024, 32768, 8, 4,
                                                                                                                 65535):
        assert ns.FOUR_TRIPS_SHAPE == (1024, 800) and ns.TALL_SHAPE == (70003, 3) and ns.WIDE_SHAPE == (3, 70001)
        assert ns.GROUP_SPLIT_PLANES == (262140, 262143, 262150)
    assert ns.PERIOD == 61 and all(ns.PERIOD % k for k in range(2, ns.PERIOD))
    for offset in (ns.PLANES, ns.MAX_GROUPS, ns.PLANES * ns.MAX_GROUPS, ns.LAYERS_PER_LAUNCH, ns.MANY_PAIRS):
        assert offset % ns.PERIOD, offset                                  # no launch offset lands on an equal plane


# ---- verification --------------------------------------------------------------------------------------------------------------
def test_layer_split_takes_a_second_launch_whose_layers_hold_sums():
    s, want = ns.verification_scene("layer_split"), ns.verification_expected("layer_split")
    n, h, w = s.forecast.shape
    layers = n * len(s.thresholds)
    launches = ns.fss_launches(layers)
    print(f"layer_split: {layers} layers in launches of {launches}; {ns.strips(h * w)} strip, trips {ns.strip_trips(h * w)}")
    assert layers == 40000 and len(launches) == 2 and launches[0] == ns.LAYERS_PER_LAUNCH and 0 < launches[1] < ns.LAYERS_PER_LAUNCH
    assert layers <= ns.SAT_MAX_LAYERS and n <= ns.CONTINGENCY_MAX_PLANES and s.scales == (1, 2, 3, 255)
    later = want.sums.reshape(layers, len(s.scales), 3)[ns.LAYERS_PER_LAUNCH:]
    filled = float((later != 0).all(axis=(1, 2)).mean())
    changing = float((later[1:] != later[:-1]).any(axis=(1, 2)).mean())
    print(f"layer_split: all three sums non-zero at every scale in {100 * filled:.1f} % of the layers from {ns.LAYERS_PER_LAUNCH} on; "
          f"{100 * changing:.1f} % of them differ from the layer before")
    assert filled > 0.5 and changing > 0.9
    # what layer0 = 0 in the second launch would add into: the first launch's layers hold other sums
    first = want.sums.reshape(layers, len(s.scales), 3)[:launches[1]]
    assert float((first != later).any(axis=(1, 2)).mean()) > 0.9
    assert np.isnan(s.forecast).any() and np.isnan(s.observed).any() and (np.isnan(s.forecast) != np.isnan(s.observed)).any()
    assert s.mask.any() and (want.counts > 0).any(axis=0).all()


def test_layer_limit_sits_at_the_limit_of_two_grids():
    s, want = ns.verification_scene("layer_limit"), ns.verification_expected("layer_limit")
    n, h, w = s.forecast.shape
    launches = ns.fss_launches(n * len(s.thresholds))
    print(f"layer_limit: {n} planes = {n * len(s.thresholds)} layers in launches of {launches}")
    assert n == ns.CONTINGENCY_MAX_PLANES and n * len(s.thresholds) == ns.SAT_MAX_LAYERS and (h, w) == (1, 3)
    assert launches == [ns.LAYERS_PER_LAUNCH, ns.SAT_MAX_LAYERS - ns.LAYERS_PER_LAUNCH] and launches[1] == 32767
    # the last plane and the last layer hold something to get wrong
    assert want.valid[-1] > 0 and want.sums[-1].any() and want.sums[ns.LAYERS_PER_LAUNCH:].any(axis=(1, 2, 3)).mean() > 0.5
    assert len(np.unique(want.counts.reshape(n, -1), axis=0)) > 5 and len(np.unique(want.valid)) == 4


def test_four_trips_walks_three_full_trips_and_a_cut_fourth():
    s, want = ns.verification_scene("four_trips"), ns.verification_expected("four_trips")
    n, h, w = s.forecast.shape
    full, cut = ns.strip_trips(h * w)
    print(f"four_trips: {h} x {w} = {h * w} pixels, {ns.strips(h * w)} strips, {full} full trips, {cut} workgroups make one more")
    assert n == 1 and ns.strips(h * w) == ns.MAX_STRIPS and full == 3 and 0 < cut < ns.MAX_STRIPS and cut == ns.MAX_STRIPS // 8
    assert h * w == 3 * ns.MAX_STRIPS * ns.BLOCK + cut * ns.BLOCK
    # the pixels of the third and of the fourth trip matter: the counts and sums of the plane cut after two trips, and after
    # three, are others
    for rows in (2 * ns.MAX_STRIPS * ns.BLOCK // w, 3 * ns.MAX_STRIPS * ns.BLOCK // w):
        part = vo.contingency(s.forecast[:, :rows], s.observed[:, :rows], s.thresholds, s.mask[:, :rows])
        assert (part.counts < want.counts).all() and part.valid[0] < want.valid[0], rows
    assert int(want.sums.max()) > 2 ** 31 and (want.sums > 0).all()
    same = float((s.forecast == s.observed).mean())
    assert 0.65 < same < 0.72 and np.isnan(s.forecast).any() and np.isnan(s.observed).any()
    assert s.mask[0, 3 * ns.MAX_STRIPS * ns.BLOCK // w:].any()            # masked pixels inside the fourth trip


def test_tall_and_wide_make_thousands_of_trips_with_a_remainder():
    tall, wide = ns.verification_scene("tall"), ns.verification_scene("wide")
    h = tall.forecast.shape[1]
    print(f"tall: {h} rows = {h // ns.COLUMN_UNROLL} unrolled trips of {ns.COLUMN_UNROLL} and {h % ns.COLUMN_UNROLL} rows")
    assert tall.forecast.shape == (1, 70003, 3) and h // ns.COLUMN_UNROLL == 8750 and h % ns.COLUMN_UNROLL == 3
    w = wide.forecast.shape[2]
    trips, last = ns.row_trips(w)
    print(f"wide: {w} columns = {trips} trips, the last of {last} pixels")
    assert wide.forecast.shape == (1, 3, 70001) and trips == 1094 and 0 < last < ns.WAVE
    want = ns.verification_expected("wide")
    row_end = np.diff(want.sat_f[0, :, :, -1], axis=1, prepend=0)         # per threshold and row: the exceedances of that row
    print(f"wide: the row carries end at {row_end.tolist()}")
    assert (row_end[0] > 2 ** 16).all() and (want.sat_o[0, 0, 0, -1] > 2 ** 16)
    assert int(ns.verification_expected("tall").sat_f[0, 0, -1, 0]) > 2 ** 16        # and the column sums


# ---- convection ----------------------------------------------------------------------------------------------------------------
def test_plane_limit_fills_the_plane_dimension_and_holds_every_class():
    s, want = ns.convection_scene("plane_limit"), ns.plane_limit_expected()
    print(f"plane_limit: {s.dbz.shape[0]} planes of {s.dbz.shape[1:]}")
    assert s.dbz.shape == (ns.CONVECTION_MAX_PLANES,) + ns.PLANE_LIMIT_SHAPE
    assert np.isnan(s.dbz).any() and s.mask.any() and 0 < want.echo.mean() < 1
    assert set(np.unique(want.centres)) == set(range(len(s.edges) + 2)) and set(np.unique(want.classes)) == {0, 1, 2}
    assert want.centres[-1].any() or want.classes[-1].any()               # the last plane holds echo
    assert np.isnan(want.bkg).any()                                       # planes without any echo


def test_wrap_row_wraps_inside_the_row():
    width, q = ns.WRAP_WIDTH, ns.WRAP_Q
    column = ns.wrap_column()
    print(f"wrap_row: q = {q}, q * w = {q * width / 2 ** 64:.4f} x 2^64, the prefix passes 2^63 at column {2 ** 63 // q} and 2^64 at "
          f"column {column}")
    assert q == 6_553_600_000_000 and q * width > 2 ** 64
    assert q * column < 2 ** 64 <= q * (column + 1) and 100_000 <= column <= width - 100_000
    uq, S, N, bkg = ns.wrap_expected("wrap_row_uniform")
    assert (uq == q).all() and np.array_equal(N, ns.wrap_window()[None, None]) and (N.astype(np.int64) * q == S).all()
    assert (bkg == np.float32(80.0)).all() and N.min() == 28 and N.max() == 55
    # the drawn row: about 2 % NaN, values from 60 to 80, and a prefix far beyond 2^53 (it reaches 2^61.8, no wrap)
    s = ns.convection_scene("wrap_row_drawn")
    dq = ns.wrap_expected("wrap_row_drawn")[0]
    total = sum(dq.ravel().tolist())
    print(f"wrap_row_drawn: the prefix ends at 2^{np.log2(float(total)):.2f}")
    assert 0.015 < np.isnan(s.dbz).mean() < 0.025 and np.nanmin(s.dbz) >= 60.0 and np.nanmax(s.dbz) <= 80.0
    assert 2 ** 61 < total < 2 ** 63 and ns.wrap_column(dq) is None


@pytest.mark.parametrize("name", ns.WRAP_ROWS)
def test_wrap_row_sums_are_what_python_integers_give(name):
    """``S`` of the oracle, whose int64 prefix wraps, against sums of ``q`` in Python's unbounded integers at 1000 columns:
    the 200 around the column where the uniform row's prefix passes 2^64, both rims, and 600 drawn."""
    q, S, N, _ = ns.wrap_expected(name)
    half = int(ns.convection_scene(name).hw[0])
    column = ns.wrap_column()
    rng = np.random.default_rng(71)
    columns = np.unique(np.concatenate([np.arange(column - 100, column + 100), np.arange(100), np.arange(ns.WRAP_WIDTH - 100, ns.WRAP_WIDTH),
                                        rng.choice(ns.WRAP_WIDTH, 640, replace=False)]))[:1000]
    assert len(columns) == 1000 and column in columns
    flat = q.ravel()
    for x in columns.tolist():
        window = flat[max(x - half, 0):min(x + half, ns.WRAP_WIDTH - 1) + 1].tolist()
        assert int(S[0, 0, x]) == sum(window), (name, x)
        assert int(N[0, 0, x]) == sum(1 for v in window if v > 0), (name, x)


# ---- accumulation and motion ---------------------------------------------------------------------------------------------------
def test_group_split_stands_at_the_limit_and_beyond_it():
    for planes, (runs, rest) in zip(ns.GROUP_SPLIT_PLANES, ([[ns.MAX_GROUPS], 0], [[ns.MAX_GROUPS], 3], [[ns.MAX_GROUPS, 2], 2])):
        got = ns.accumulation_runs(planes)
        print(f"group_split: {planes} planes = launches of {got[0]} groups and a remainder of {got[1]} planes")
        assert got == (runs, rest)
        assert planes * 6 < 2 ** 31                                       # a legal call
    h, w = ns.GROUP_SPLIT_SHAPE
    assert h <= ns.TILE_H and w <= ns.TILE_W                              # one tile: gridDim.x == 1, gridDim.y the group count
    for method in ns.GROUP_SPLIT_METHODS:
        s, want = ns.group_split_scene(method), ns.group_split_expected(method)
        assert s.prev.shape == (ns.PERIOD, h, w) and (s.n_steps, s.substeps, s.min_steps) == (3, 2, 2) and s.method == method
        assert ns.distinct(want.out) and ns.distinct(s.prev) and ns.distinct(s.next)
        assert len(np.unique(want.steps)) == 4 and acs.is_fill(want.out, s.fill).any() and np.isinf(want.out).any()
        assert want.both and want.only_prev and want.only_next and want.neither
    assert ns.group_split_expected("nearest").out.tobytes() != ns.group_split_expected("bilinear").out.tobytes()


def test_many_pairs_has_a_period_of_distinct_results():
    prev, nxt = ns.many_pairs_levels()
    m = ns.many_pairs_match()
    nby, nbx = m.valid.shape[1:]
    print(f"many_pairs: {ns.MANY_PAIRS} pairs x {nby} x {nbx} blocks = {ns.MANY_PAIRS * nby * nbx} workgroups; "
          f"{100 * m.valid.mean():.1f} % of the base blocks qualify")
    assert prev.shape == (ns.PERIOD,) + ns.PAIR_SHAPE and (nby, nbx) == (2, 4) and ns.MANY_PAIRS % ns.PERIOD and ns.MANY_PAIRS > 4096
    assert m.valid.mean() > 0.9 and not m.valid.all() and np.isnan(m.score).any()
    assert ns.distinct(m.score) and ns.distinct(m.motion) and len(np.unique(m.disp.reshape(-1, 2), axis=0)) >= 20
    assert not np.isnan(m.score).all(axis=(1, 2)).any()                   # no pair without a vector
    planes, motion, lat = ns.advect_base()
    assert planes.shape == (ns.PERIOD,) + ns.PAIR_SHAPE and motion.shape == (lat.ny, lat.nx, 2) == (2, 4, 2)
    for method in ns.ADVECT_METHODS:
        want = ns.advect_expected(method)
        assert want.shape == (len(ns.ADVECT_LEADS), ns.PERIOD) + ns.PAIR_SHAPE
        assert all(ns.distinct(lead) for lead in want) and (want == np.float32(ns.ADVECT_FILL)).any()
    assert np.isnan(ns.advect_expected("nearest")).any()


# ---- one plane or layer more than gridDim.y holds is refused on the host ---------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import radar_processor_amd as rg
    return rg.load_library(require_device=False)


EINVAL = -1
P = 4096                                       # a pointer that is never followed: every call below fails its checks first
FAR = 1 << 40


def _refused(lib, status, limit):
    assert status == EINVAL and str(limit).encode() in lib.rg_last_error(), (status, lib.rg_last_error())


def test_verification_refuses_one_more_than_the_grid_holds(lib):
    thr = (ctypes.c_float * 8)(*range(8))
    over = ns.CONTINGENCY_MAX_PLANES + 1
    _refused(lib, lib.rg_contingency_f32(P, P, 0, over, 1, 3, thr, 1, FAR, 2 * FAR, 0), ns.CONTINGENCY_MAX_PLANES)
    assert b"planes" in lib.rg_last_error()
    over = ns.SAT_MAX_LAYERS + 1
    assert over % 8 == 0
    for planes, n_thr in ((over, 1), (over // 8, 8)):
        _refused(lib, lib.rg_exceedance_sat_i32(P, 0, 0, planes, 1, 3, thr, n_thr, FAR, 0), ns.SAT_MAX_LAYERS)
        assert b"layers" in lib.rg_last_error()


def test_convection_refuses_one_more_plane_than_the_grid_holds(lib):
    over, limit = ns.CONVECTION_MAX_PLANES + 1, ns.CONVECTION_MAX_PLANES
    hw = (ctypes.c_int32 * 128)(1, 1)
    ry = (ctypes.c_int32 * 1)(1)
    edges = (ctypes.c_double * 1)(25.0)
    _refused(lib, lib.rg_echo_table_f32(P, 0, over, 2, 3, 5.0, FAR, 1 << 30, 0), limit)
    _refused(lib, lib.rg_disk_background(FAR, over, 2, 3, hw, 1, 0, 0, P, 0), limit)
    _refused(lib, lib.rg_convective_centres_f32(P, 0, 2 * FAR, over, 2, 3, 5.0, 40.0, 10.0, 180.0, edges, 2, FAR, 0), limit)
    _refused(lib, lib.rg_convective_area_u8(P, 2 * FAR, 0, over, 2, 3, 5.0, 1, hw, ry, 3 * FAR, 1 << 30, FAR, 0), limit)
    assert lib.rg_echo_table_bytes(over, 2, 3) == EINVAL and lib.rg_convective_area_workspace_bytes(over, 2, 3, 1) == EINVAL
    # the limit itself is a size question only: the byte counts of the scene
    assert lib.rg_echo_table_bytes(limit, 2, 3) == limit * 2 * 4 * 16 and lib.rg_convective_area_workspace_bytes(limit, 2, 3, 5) > 0


def test_the_python_functions_refuse_the_same_counts():
    import radar_processor_amd as rg
    over = np.zeros((ns.CONTINGENCY_MAX_PLANES + 1, 1, 3), dtype=np.float32)
    eighth = over[:len(over) // 8]
    with pytest.raises(ValueError, match=str(ns.CONTINGENCY_MAX_PLANES)):
        rg.contingency_device(over, over, (18.0,))
    for call in (lambda: rg.exceedance_sat_device(over, (18.0,)), lambda: rg.exceedance_sat_device(eighth, tuple(range(8))),
                 lambda: rg.fss_device(over, over, (18.0,), (1,)), lambda: rg.fss_device(eighth, eighth, tuple(range(8)), (1,)),
                 lambda: rg.neighbourhood_fraction_device(over, (18.0,), 3), lambda: rg.verify_nowcast(over, over, (18.0,), (1,))):
        with pytest.raises(ValueError, match=str(ns.SAT_MAX_LAYERS)):
            call()
    for call in (lambda: rg.convective_stratiform_device(over, dx=400.0), lambda: rg.echo_background_device(over, dx=400.0)):
        with pytest.raises(ValueError, match=str(ns.CONVECTION_MAX_PLANES)):
            call()


def test_the_restated_background_of_one_row_needs_only_the_first_half_width():
    """What ``wrap_row`` relies on: in a plane of one row the footprint's other rows fall outside, whatever their widths."""
    s = ns.convection_scene("wrap_row_drawn")
    part = s.dbz[:, :, :5000]
    whole, first = co.background(part, s.hw), co.background(part, s.hw[:1])
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(whole, first)) and len(s.hw) > 20 and s.hw[0] == 27
