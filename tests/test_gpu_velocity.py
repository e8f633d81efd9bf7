"""The velocity kernels on the device against the NumPy restatement (tests/velocity_oracle.py): every output is EQUAL -- the
regions, the sorted edge set with counts and sums, the folds, and the velocity bit for bit.  The shapes are the smallest that can
go wrong: single rays and gates, rows of 63 / 64 / 65 gates so that wavefronts straddle rays, two sweeps under one wavefront,
borders that run along a ray (runs of 64 lanes, one insertion) and across it (no runs), a checkerboard that fills the table."""
import ctypes

import numpy as np
import pytest

from radar_processor_amd import _native

import velocity_oracle as vo
import velocity_scenes as vs

pytestmark = pytest.mark.gpu


def _np(t):
    return t.cpu().numpy()


def _edge_rows(e):
    """RegionEdges -> int64 [n][4], sorted by (lo, hi) as the wrapper returns them."""
    return np.concatenate([_np(e.pairs).astype(np.int64).reshape(-1, 2), _np(e.count).astype(np.int64)[:, None], _np(e.sum)[:, None]], axis=1)


@pytest.mark.parametrize("name", sorted(vs.scenes()))
def test_every_output_of_the_chain_equals_the_restatement(name):
    import radar_processor_amd as rg
    s, ref = vs.scenes()[name], vs.reference(name)
    want = vo.regions(s.vel, s.nyquist, s.n_bands, s.mask, s.wrap)
    # the split
    split = _np(rg.split_velocity_device(s.vel, s.nyquist, n_bands=s.n_bands, mask=s.mask))
    want_split = vo.split(s.vel, s.nyquist, s.n_bands, s.mask)
    np.testing.assert_array_equal(vo.bits(split), vo.bits(want_split.reshape(split.shape)))
    # the regions, their sizes and cell_ptr
    reg = rg.velocity_regions_device(s.vel, s.nyquist, n_bands=s.n_bands, mask=s.mask, wrap_rays=s.wrap)
    assert reg.n_regions == ref.n_regions == len(want.sizes)
    np.testing.assert_array_equal(_np(reg.regions), ref.regions)
    np.testing.assert_array_equal(_np(reg.sizes), want.sizes)
    np.testing.assert_array_equal(_np(reg.cell_ptr), want.cell_ptr)
    # the edge table: complete, and the SET equals the restatement's
    edges = rg.region_edges_device(s.vel, reg.regions, wrap_rows=s.wrap)
    assert edges.totals == (len(ref.edges), 0)
    np.testing.assert_array_equal(_edge_rows(edges), ref.edges)
    # the chain: folds and velocity
    got = rg.dealias_velocity_device(s.vel, s.nyquist, n_bands=s.n_bands, mask=s.mask, wrap_rays=s.wrap)
    assert (got.n_regions, got.n_edges) == (ref.n_regions, len(ref.edges))
    np.testing.assert_array_equal(_np(got.regions), ref.regions)
    np.testing.assert_array_equal(_np(got.folds), ref.folds)
    np.testing.assert_array_equal(vo.bits(_np(got.velocity)), vo.bits(ref.velocity))
    assert got.velocity.shape == s.vel.shape and got.folds.dtype == __import__("torch").int32
    if name in vs.RECOVERING:
        ok = vo.valid(s.vel)
        np.testing.assert_array_equal(_np(got.folds)[ok], s.truth_folds[ok])
        restored = (s.vel.astype(np.float64) + s.truth_folds * (2.0 * float(s.nyquist))).astype(np.float32)
        np.testing.assert_array_equal(vo.bits(_np(got.velocity)[ok]), vo.bits(restored[ok]))
        assert np.isnan(_np(got.velocity)[~ok]).all()


def test_the_numpy_form_returns_arrays():
    import radar_processor_amd as rg
    s, ref = vs.scenes()["wind_24x40"], vs.reference("wind_24x40")
    got = rg.dealias_velocity(s.vel, s.nyquist, n_bands=s.n_bands, wrap_rays=s.wrap)
    assert all(isinstance(a, np.ndarray) for a in got[:3])
    np.testing.assert_array_equal(vo.bits(got.velocity), vo.bits(ref.velocity))
    np.testing.assert_array_equal(got.folds, ref.folds)


@pytest.mark.parametrize("axis,R,wrap", [("ray", 18, True), ("ray", 18, False), ("gate", 6, True), ("gate", 6, False), ("ray", 2, True),
                                         ("ray", 3, True)])
def test_runs_along_a_border_are_combined_and_the_sums_pass_2_to_the_32(axis, R, wrap):
    """Two regions split along one boundary of G = 200 gates: along a ray boundary the 200 pairs of a border arrive as runs of up
    to 64 lanes and the run's last lane inserts; along a gate boundary every pair is alone in its wavefront."""
    import radar_processor_amd as rg
    values, region = vs.two_regions(axis, R=R)
    want = vo.edges(values, region, wrap)
    assert abs(int(want[0, 3])) > 2 ** 32 or want[0, 2] < 200
    got = rg.region_edges_device(values, region, wrap_rows=wrap)
    assert got.totals == (1, 0)
    np.testing.assert_array_equal(_edge_rows(got), want)


@pytest.mark.parametrize("shape,ids,seed", [((1, 1, 1), 3, 0), ((1, 1, 70), 3, 1), ((1, 70, 1), 3, 2), ((3, 5, 65), 6, 3), ((2, 3, 64), 4, 4),
                                             ((4, 7, 63), 9, 5), ((1, 130, 129), 40, 6)])
def test_the_edge_kernel_is_generic_any_values_and_any_region_ids(shape, ids, seed):
    """Region ids that are no connected sets, 0 and negative ids, values that are not valid: equal to the double loop."""
    import radar_processor_amd as rg
    rng = np.random.default_rng(seed)
    region = rng.integers(-1, ids + 1, shape).astype(np.int32)
    region[rng.random(shape) < 0.3] = rng.integers(1, ids + 1)                      # some larger patches of one id
    values = rng.uniform(-16384.0, 16384.0, shape).astype(np.float32)
    odd = rng.random(shape) < 0.1
    values[odd] = rng.choice(np.array([np.nan, np.inf, -np.inf, 16384.5, -3e38, 16384.0, -16384.0], np.float32), int(odd.sum()))
    for wrap in (False, True):
        want = vo.edges(values, region, wrap)
        got = rg.region_edges_device(values, region, wrap_rows=wrap, max_edges=ids * ids)
        assert got.totals == (len(want), 0)
        np.testing.assert_array_equal(_edge_rows(got), want)


def test_a_checkerboard_fills_the_table_and_a_small_table_reports_the_shortfall():
    """Every gate its own region, every neighbour pair an edge: the chain holds them all.  With max_edges = 8 the table has 64
    slots: totals says so, the call still succeeds, and every row written is a true edge with its full count and sum."""
    import radar_processor_amd as rg
    s = vs.checkerboard()
    ref = vo.dealias(s.vel, s.nyquist, s.n_bands, None, s.wrap)
    got = rg.dealias_velocity_device(s.vel, s.nyquist, n_bands=s.n_bands, wrap_rays=s.wrap)
    assert (got.n_regions, got.n_edges) == (s.vel.size, len(ref.edges))
    np.testing.assert_array_equal(_np(got.regions), ref.regions)
    np.testing.assert_array_equal(_np(got.folds), ref.folds)
    np.testing.assert_array_equal(vo.bits(_np(got.velocity)), vo.bits(ref.velocity))
    full = rg.region_edges_device(s.vel, ref.regions, wrap_rows=s.wrap)
    np.testing.assert_array_equal(_edge_rows(full), ref.edges)
    small = rg.region_edges_device(s.vel, ref.regions, wrap_rows=s.wrap, max_edges=8)
    held, dropped = small.totals
    assert held == 64 and dropped > 0                        # 64 slots, all taken: 8 < held reports the shortfall
    rows = _edge_rows(small)
    assert len(rows) == 8 and len({(lo, hi) for lo, hi, _, _ in rows.tolist()}) == 8
    truth = {(lo, hi): (c, t) for lo, hi, c, t in ref.edges.tolist()}
    for lo, hi, c, t in rows.tolist():
        assert truth[(lo, hi)] == (c, t)


def test_more_sweeps_than_one_launch_carries():
    """70 sweeps, each with a Nyquist velocity of its own: the split and the apply take two launches."""
    import radar_processor_amd as rg
    S, R, G = 70, 2, 5
    rng = np.random.default_rng(9)
    nyq = np.linspace(4.0, 30.0, S)
    vel = (rng.uniform(-1.0, 1.0, (S, R, G)) * nyq[:, None, None]).astype(np.float32)
    split = _np(rg.split_velocity_device(vel, nyq, n_bands=4))
    np.testing.assert_array_equal(vo.bits(split), vo.bits(vo.split(vel, nyq, 4)))
    region = rng.integers(0, 9, (S, R, G)).astype(np.int32)
    lut = rng.integers(-3, 4, 7).astype(np.int32)
    out, folds = rg.apply_folds_device(vel, region, lut, nyq, return_folds=True)
    want, want_folds = vo.apply(vel, region, lut, nyq)
    np.testing.assert_array_equal(vo.bits(_np(out)), vo.bits(want))
    np.testing.assert_array_equal(_np(folds), want_folds)
    assert np.isnan(want[region == 8]).all() and np.isnan(want[region == 0]).all()          # id 8 is above the 7 regions


def test_apply_in_place_ids_above_n_regions_and_values_that_are_not_finite():
    import torch
    import radar_processor_amd as rg
    lib = rg.load_library()
    dev = torch.device("cuda", 0)
    S, R, G = 2, 3, 67
    rng = np.random.default_rng(3)
    vel = rng.uniform(-12.0, 12.0, (S, R, G)).astype(np.float32)
    vel[0, 0, :4] = [np.nan, np.inf, -np.inf, 3e38]
    vel[1, 2, 5] = -np.nan
    region = rng.integers(-2, 14, (S, R, G)).astype(np.int32)
    region[0, 0, :4] = [1, 2, 3, 4]
    region[1, 2, 5] = 2
    lut = rng.integers(-40, 41, 11).astype(np.int32)
    lut[3] = 2 ** 31 - 1
    nyq = (ctypes.c_double * S)(11.5, 7.25)
    want, want_folds = vo.apply(vel, region, lut, (11.5, 7.25))
    v, r, l = (torch.from_numpy(a).to(dev) for a in (vel, region, lut))
    folds = torch.full((S, R, G), -77, dtype=torch.int32, device=dev)
    assert lib.rg_velocity_apply_folds_f32(_native.ptr(v), _native.ptr(r), _native.ptr(l), 11, S, R, G, nyq, _native.ptr(v),
                                           _native.ptr(folds), _native.stream_ptr()) == 0, lib.rg_last_error().decode()
    np.testing.assert_array_equal(vo.bits(_np(v)), vo.bits(want))
    np.testing.assert_array_equal(_np(folds), want_folds)
    assert np.isnan(want[region > 11]).all() and np.isnan(want[region <= 0]).all() and (want_folds[region > 11] == 0).all()
    assert vo.bits(want)[0, 0, 0] == 0x7FC00000 and want[0, 0, 1] == np.inf and want_folds[0, 0, 0] == 0 and want_folds[0, 0, 1] == lut[1]
    # no regions at all: NaN everywhere, through the wrapper and a NULL table
    out = rg.apply_folds_device(vel, np.zeros_like(region), np.zeros(0, np.int32), (11.5, 7.25))
    assert (vo.bits(_np(out)) == 0x7FC00000).all()


def test_flattening_takes_the_lowest_band_and_ignores_labels_beyond_the_count():
    """rg_velocity_regions_i32 over labels no labeller wrote: two bands labelled at one gate, labels above the plane's count."""
    import torch
    import radar_processor_amd as rg
    lib = rg.load_library()
    dev = torch.device("cuda", 0)
    S, B, R, G = 2, 3, 3, 66
    rng = np.random.default_rng(5)
    labels = rng.integers(-1, 6, (S, B, R, G)).astype(np.int32)
    cell_ptr = np.cumsum([0, 3, 0, 5, 2, 4, 1]).astype(np.int32)
    want = vo.flatten(labels, cell_ptr, B)
    assert (want == 0).any() and (want > 0).sum() > 100 and want.max() <= 15
    lab, ptr = torch.from_numpy(labels).to(dev), torch.from_numpy(cell_ptr).to(dev)
    out = torch.full((S, R, G), -5, dtype=torch.int32, device=dev)
    assert lib.rg_velocity_regions_i32(_native.ptr(lab), _native.ptr(ptr), S, R, G, B, _native.ptr(out), _native.stream_ptr()) == 0
    np.testing.assert_array_equal(_np(out), want)


def test_empty_volumes():
    import radar_processor_amd as rg
    got = rg.dealias_velocity_device(np.zeros((2, 4, 0), np.float32), 10.0)
    assert got.velocity.shape == (2, 4, 0) and (got.n_regions, got.n_edges) == (0, 0)
    got = rg.dealias_velocity_device(np.full((4, 9), np.nan, np.float32), 10.0)
    assert np.isnan(_np(got.velocity)).all() and (got.n_regions, got.n_edges) == (0, 0) and (_np(got.folds) == 0).all()
    e = rg.region_edges_device(np.zeros((3, 0), np.float32), np.zeros((3, 0), np.int32), wrap_rows=True, max_edges=4)
    assert e.totals == (0, 0) and e.pairs.shape == (0, 2)
