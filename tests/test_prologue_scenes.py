"""The generators of tests/prologue_scenes.py hold what tests/test_gpu_prologue.py relies on (no GPU needed): every planted
case is present, the references agree with brute force, the free band of the per-level lists cannot hide a failure, and the
vertical scene's planted gates are neighbours in the float64 oracle."""
import numpy as np
import pytest

import prologue_scenes as ps
from oracle import radar_grid_oracle as oracle


def test_constants_are_the_build_s():
    from radar_processor_amd import _native
    from radar_processor_amd.gridding import _stride_for
    assert ps.EXCLUDED_BITS == _native.RG_EXCLUDED_BITS and tuple(_native.GATE_OPS) == ps.GATE_OPS
    for n in range(1, _native.RG_MAX_FIELDS + 1):
        assert ps.strides_for(n)[0] == _stride_for(n)
    assert ps.strides_for(1) == (1, 2, 4, 8) and ps.strides_for(3) == (4, 8) and ps.strides_for(8) == (8,)


def test_special_values_and_the_pack_reference():
    sp = ps.special_values()
    assert len(set(sp.values())) == len(sp) == 13
    f = ps.from_bits(list(sp.values()))
    assert int(np.isnan(f).sum()) == 6 and int(np.isinf(f).sum()) == 2
    assert sp["sentinel"] == ps.EXCLUDED_BITS and sp["neg_sentinel"] == ps.EXCLUDED_BITS | 0x80000000
    assert list(ps.is_signalling(list(sp.values()))) == [k == "snan" for k in sp]
    assert f[list(sp).index("denormal")] == np.float32(1e-45) and f[list(sp).index("huge")] == np.float32(3.0e38)
    # two fields in stride 4: field 0 masked by a byte of 0x80 on gate 1, shared mask 2 on gate 2, the sentinel unmasked on gate 3
    a = ps.from_bits([sp["neg_zero"], sp["payload_nan"], 0x3F800000, sp["sentinel"], sp["snan"]])
    b = ps.from_bits([sp["sentinel"], sp["neg_sentinel"], sp["denormal"], sp["pos_inf"], sp["qnan"]])
    m0 = np.array([0, 0x80, 0, 0, 0], dtype=np.uint8)
    shared = np.array([0, 0, 2, 0, 0], dtype=np.uint8)
    got = ps.pack_fields_ref([a, b], [m0, None], shared, 4)
    e, q = ps.EXCLUDED_BITS, ps.CANONICAL_NAN
    assert got.dtype == np.uint32 and got.tolist() == [
        [sp["neg_zero"], q, e, e], [e, sp["neg_sentinel"], e, e], [e, e, e, e], [q, sp["pos_inf"], e, e],
        [sp["snan"], sp["qnan"], e, e]]
    loose = ps.pack_loose_slots([a, b], [m0, None], shared, 4)
    assert np.argwhere(loose).tolist() == [[0, 1], [3, 0], [4, 0]]
    assert np.array_equal(ps.pack_fields_ref([a], None, None, 1)[:, 0], np.where(ps.bits(a) == e, q, ps.bits(a)))


def test_gate_mask_cases_hold_their_edges():
    cases = ps.gate_mask_cases()
    assert {c[0] for c in cases} == set(ps.GATE_OPS) and len(cases) == 27
    n_equal_edges = 0
    for op, a, b, d in cases:
        assert isinstance(a, float) and isinstance(b, float) and d.dtype == np.float32
        a32, b32 = np.float32(a), np.float32(b)
        db = set(ps.bits(d).tolist())
        for t in (a32, b32):                                   # the thresholds and their neighbours on both sides
            for v in (t, np.nextafter(t, ps.INF32), np.nextafter(t, -ps.INF32)):
                assert int(ps.bits([v])[0]) in db
        sp = ps.special_values()
        for k in ("pos_zero", "neg_zero", "pos_inf", "neg_inf", "denormal", "neg_denormal", "qnan", "neg_qnan", "sentinel",
                  "snan"):
            assert sp[k] in db, k
        want = ps.gate_mask_ref(op, d, a, b)
        assert want.dtype == bool and want.shape == d.shape
        assert not want[np.isnan(d)].any() or op == "invalid"
        if op == "equal" and b32 > 0 and np.isfinite(b32) and b32 > np.float32(1e-30):
            with np.errstate(invalid="ignore"):
                diff = np.abs(d - a32)
            assert diff.dtype == np.float32
            at, below, above = diff == b32, diff == np.nextafter(b32, -ps.INF32), diff == np.nextafter(b32, ps.INF32)
            # the lattice around a +- b straddles b on both ends; |d - a| == b itself is not excluded (strict <)
            near = np.abs(diff.astype(np.float64) - float(b32)) < 1e-6
            assert (want & near).sum() >= 2 and (~want & near).sum() >= 2, (a, b)
            assert not want[at].any() and want[below].all() and not want[above].any()
            if a == 0.0:                                       # |d| itself: exactly b and one ulp either side
                assert at.sum() >= 2 and below.sum() >= 2 and above.sum() >= 2
            n_equal_edges += int(at.sum())
        if op in ("below", "above") and a == 0.0:              # +-0 against a = 0: neither below nor above
            assert not want[d == 0].any() and int((d == 0).sum()) >= 2
    assert n_equal_edges >= 6
    # thresholds float32 cannot represent are in the list, as Python floats
    assert any(a == 0.1 for _, a, _, _ in cases) and any(a == 0.8 for _, a, _, _ in cases)
    assert np.float64(np.float32(0.1)) != 0.1 and np.float64(np.float32(0.8)) != 0.8
    # the strict comparison is what the data can tell from a non-strict one
    op, a, b, d = cases[1]
    assert (op, a) == ("below", 0.8) and int((d == np.float32(0.8)).sum()) >= 1 and not ps.gate_mask_ref(op, d, a, b)[d == np.float32(0.8)].any()


def _planted_counts(s):
    return {c: len(v) for c, v in s.planted.items()}


def test_binning_scenes_hold_every_planted_case():
    scenes = ps.binning_scenes()
    assert sorted(s.n for s in scenes) == [0, 1, 255, 256, 257, 257, 300, 4999, 5000, 5003]
    planted_scenes = [s for s in scenes if s.name.startswith("planted_")]
    assert len(planted_scenes) == 5 and {s.toa for s in planted_scenes} == {6000.0, 17000.0}
    for s in planted_scenes:
        c = s.cells
        assert (c.ncx, c.ncy) == (7, 3) and c.ncx != c.ncy and c.x0 % c.cell == 0 and c.y0 % c.cell == 0
        assert np.log2(c.cell) == int(np.log2(c.cell)) and np.float32(s.alt) == s.alt != 0.0
        z_rel, keep, cell = ps.gate_cells(s.gx, s.gy, s.gz, s.alt, s.toa, c)
        counts = _planted_counts(s)
        for case, (kept, need) in ps.PLANTED.items():
            assert counts.get(case, 0) >= need, (s.name, case, counts)
            assert (keep[s.planted[case]] == kept).all(), (s.name, case)
        print(f"{s.name}: {counts}; {int(keep.sum())} of {s.n} gates kept")
        # where the planted gates land: the boundary itself opens cell k, one ulp below it lies in cell k - 1
        assert sorted(cell[s.planted["x_boundary"]]) == [1, 2, 3, 4, 5, 6]
        # (except below x = 0: the negative denormal minus x0 rounds to the boundary in float64 and stays in cell 4)
        assert sorted(cell[s.planted["x_below_boundary"]]) == [0, 1, 2, 4, 4, 5]
        assert sorted(cell[s.planted["y_boundary"]]) == [8, 15] and sorted(cell[s.planted["y_below_boundary"]]) == [1, 8]
        assert cell[s.planted["x_at_origin"]] == 0 and cell[s.planted["x_inside_origin"]] == 0
        assert cell[s.planted["x_inside_end"]] == 6 and cell[s.planted["y_inside_end"]] == 14
        top = np.float32(min(s.toa, c.z_hi))
        assert (z_rel[s.planted["z_at_top"]] == top).all()
        assert (z_rel[s.planted["z_above_top"]] == np.nextafter(top, ps.INF32)).all()
        assert (z_rel[s.planted["z_at_lo"]] == np.float32(c.z_lo)).all()
        assert (z_rel[s.planted["z_below_lo"]] == np.nextafter(np.float32(c.z_lo), -ps.INF32)).all()
        bad = s.planted["nonfinite"]
        for v in (s.gx, s.gy, s.gz):
            assert int(np.isnan(v[bad]).sum()) == 1 and int(np.isposinf(v[bad]).sum()) == 1 and int(np.isneginf(v[bad]).sum()) == 1
        dup = s.planted["duplicates"]
        assert len({(s.gx[i], s.gy[i], s.gz[i]) for i in dup}) == 1 and len(set(cell[dup])) == 1
        # an empty cell in the middle, an empty last cell, every other cell populated, gates dropped on every side
        per_cell = np.bincount(cell[keep], minlength=c.ncx * c.ncy)
        assert per_cell[ps.EMPTY_MIDDLE] == 0 and per_cell[-1] == 0 and (np.delete(per_cell, [ps.EMPTY_MIDDLE, 20]) > 0).all()
        assert 0.3 < keep.mean() < 0.95
    by_name = {s.name: s for s in scenes}
    assert not ps.gate_cells(*_args(by_name["all_dropped"]))[1].any()
    assert ps.gate_cells(*_args(by_name["single"]))[1].all()
    one = by_name["one_cell"]
    assert (one.cells.ncx, one.cells.ncy) == (1, 1) and 0 < ps.gate_cells(*_args(one))[1].sum() < one.n
    odd = by_name["odd_cells"]
    assert odd.cells.cell == 731.7 and np.log2(odd.cells.cell) != int(np.log2(odd.cells.cell))


def _args(s):
    return s.gx, s.gy, s.gz, s.alt, s.toa, s.cells


def test_bin_gates_ref_agrees_with_a_per_gate_loop():
    for name in ("planted_257_toa6000", "one_cell", "empty", "all_dropped"):
        s = next(x for x in ps.binning_scenes() if x.name == name)
        rec, start = ps.bin_gates_ref(*_args(s))
        order, want_start = ps.brute_force_bins(s)
        assert np.array_equal(rec["index"], order) and np.array_equal(start, want_start)
        assert start.dtype == np.int32 and start.shape == (s.cells.ncx * s.cells.ncy + 1,) and start[-1] == rec.size
        z_rel = (s.gz - np.float32(s.alt)).astype(np.float32)
        assert np.array_equal(rec["x"], ps.bits(s.gx)[order]) and np.array_equal(rec["z"], ps.bits(z_rel)[order])
    # the order inside a cell is the gate index: the five duplicates come out ascending and adjacent
    s = next(x for x in ps.binning_scenes() if x.name == "planted_257_toa6000")
    rec, _ = ps.bin_gates_ref(*_args(s))
    pos = np.nonzero(np.isin(rec["index"], s.planted["duplicates"]))[0]
    assert np.array_equal(rec["index"][pos], s.planted["duplicates"])


@pytest.mark.parametrize("min_radius,beam_factor", ps.LEVEL_PARAMS)
def test_level_scenes_partition_and_free_band(min_radius, beam_factor):
    for alt in ps.LEVEL_ALTS:
        s = ps.level_scene(min_radius, beam_factor, alt)
        assert s.min_radius >= 250.0 and 0.0 <= s.beam_factor < 0.5
        must, may, never = ps.level_lists_ref(*_args(s), s.zc, s.min_radius, s.beam_factor)
        assert must.shape == (len(s.zc), s.n)
        assert np.array_equal(must.astype(int) + may.astype(int) + never.astype(int), np.ones(must.shape, dtype=int))
        _, keep, _ = ps.gate_cells(*_args(s))
        assert never[:, ~keep].all() and (~keep).sum() > 100
        # the planted gates: just inside the bound -> must, just outside -> never, at their own level
        for case, table in (("inside", must), ("outside", never)):
            idx = s.planted[case]
            assert len(idx) == ps.N_LEVEL_EDGE and keep[idx].all()
            assert all(table[s.planted_level[int(i)], i] for i in idx), case
        n_must, n_may = int(must.sum()), int(may.sum())
        print(f"{s.name}: {n_must} must, {n_may} may, {int(never.sum())} never")
        assert n_must >= 500 and n_may <= 0.01 * n_must            # the free band cannot hide a failure
        # the reference order of the must set is (level, cell, gate index) with records as in the single list
        rec, start = ps.level_order_ref(*_args(s), must)
        n_cells = s.cells.ncx * s.cells.ncy
        assert rec.size == n_must and start.shape == (len(s.zc) * n_cells + 1,) and start[-1] == n_must
        assert np.array_equal(np.diff(start[::n_cells]), must.sum(axis=1))
        _, _, cell = ps.gate_cells(*_args(s))
        lev = np.searchsorted(start[::n_cells], np.arange(rec.size), side="right") - 1
        key = np.stack([lev, cell[rec["index"]], rec["index"]])
        assert (np.lexsort(key[::-1]) == np.arange(rec.size)).all()


def test_on_bound_scene_sits_on_the_bound():
    """Every planted |dz| is exactly 9/11 of the gate's height; the float64 R_g of the reference puts most of the pairs on or
    inside the bound, and another equally valid float64 order of the same expression, |g| * (bf / (1 - bf)), disagrees on
    many of them: a list built without the documented inflation cannot hold every required pair of both."""
    s = ps.on_bound_scene()
    o = ps.ON_BOUND
    must, may, never = ps.level_lists_ref(*_args(s), s.zc, s.min_radius, s.beam_factor)
    assert ps.gate_cells(*_args(s))[1].all() and len(s.pairs) >= 200
    k, g = np.array(s.pairs).T
    z, dz = s.gz[g].astype(np.float64), np.abs(s.gz[g].astype(np.float64) - s.zc[k].astype(np.float64))
    assert np.array_equal(dz * o["den"], z * o["num"]) and (dz > s.min_radius).all()
    assert not never[k, g].any()
    other_order = z * (s.beam_factor / (1.0 - s.beam_factor))
    n_must, n_split = int(must[k, g].sum()), int((must[k, g] & (dz > other_order)).sum())
    print(f"on-bound scene: {len(s.pairs)} pairs, {n_must} required by the reference, {n_split} of those outside the bound "
          f"in the other float64 order; {int(may.sum())} of {int((must | may).sum())} listable pairs in the free band")
    assert n_must >= 100 and n_split >= 10
    assert may.sum() <= 0.01 * must.sum()


@pytest.mark.parametrize("beam_factor", ps.VERTICAL_BEAMS)
@pytest.mark.parametrize("eps", ps.VERTICAL_EPS)
def test_vertical_scene_plants_neighbours(beam_factor, eps):
    s = ps.vertical_rim_scene(beam_factor, eps)
    nz, ny, nx = s.shape
    assert ny % 2 == 1 and nx % 2 == 1 and s.limits[1][0] == -s.limits[1][1] and s.limits[2][0] == -s.limits[2][1]
    assert len(s.planted) == 2 * nz and (s.gx[:2 * nz] == 0).all() and (s.gy[:2 * nz] == 0).all()
    ip, idx, _ = oracle.build_geometry(s.gx, s.gy, s.gz, s.shape, s.limits, min_radius=s.min_radius,
                                       beam_factor=s.beam_factor, weighting="nearest")
    for v, g in s.planted:
        assert g in idx[ip[v]:ip[v + 1]], (v, g)
    # the margin to the rim shrinks with eps, down to the float32 spacing of the heights (5e-4 .. 1e-3 m here)
    zc = np.linspace(*s.limits[0], nz, dtype="float32").astype(np.float64)
    r_v = np.repeat(zc * s.beam_factor, 2)
    assert (s.margins > 0).all() and (s.margins <= r_v * eps + 2e-3).all()
    # ... and with it the margin of the per-level bound for the gate below its voxel: R_g - |dz| = (r_v - |dz|) / (1 - bf)
    z = s.gz[:2 * nz:2].astype(np.float64)
    r_g = z * s.beam_factor / (1.0 - s.beam_factor)
    slack = r_g - (zc - z)
    assert (slack > 0).all() and np.allclose(slack, s.margins[::2] / (1.0 - s.beam_factor), rtol=0, atol=1e-8)
    print(f"bf {beam_factor} eps {eps}: smallest R_g - |dz| = {slack.min():.3e} m")


def test_sentinel_scene_reaches_many_voxels():
    s = ps.sentinel_scene()
    assert int(s.hot.sum()) == 40 and not (s.hot & s.mask).any()
    assert (ps.bits(s.a)[s.hot] == ps.EXCLUDED_BITS).all() and (ps.bits(s.a_ref)[s.hot] == ps.CANONICAL_NAN).all()
    assert np.array_equal(ps.bits(s.a)[~s.hot], ps.bits(s.a_ref)[~s.hot])
    ip, idx, w = oracle.build_geometry(s.gx, s.gy, s.gz, s.shape, s.limits, min_radius=s.min_radius,
                                       beam_factor=s.beam_factor)
    row = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    touched = np.unique(row[s.hot[idx]])
    want = oracle.csr_apply_f64(ip, idx, w, s.a_ref, s.mask, s.shape).ravel()
    assert touched.size >= 50 and np.isnan(want[touched]).all()
    without = oracle.csr_apply_f64(ip, idx, w, s.a_ref, s.mask | s.hot, s.shape).ravel()
    assert int(np.isfinite(without[touched]).sum()) >= 50            # dropping the gate instead would give a number there
    print(f"sentinel scene: {touched.size} voxels with a sentinel-valued neighbour")
