"""``oracle.closest_gate_choice`` -- the exact prediction of the closest-gate mode of ``rg_roi_grid_f32`` -- on hand-made
cases, against the older ``oracle.closest_gate_grid`` and against float64 (the derived bound on the winner's distance), and
the conditions tests/closest_scenes.py's scenes must meet so that tests/test_gpu_closest.py exercises what it claims to.
No GPU needed."""
import numpy as np
import pytest

import closest_scenes as cs
from oracle import radar_grid_oracle as oracle
from oracle import roi_rim

F32 = np.float32
# one voxel at (x, y, z) = (0, 0, 1000)
ONE = dict(grid_shape=(1, 1, 1), grid_limits=((1000.0, 1000.0), (0.0, 0.0), (0.0, 0.0)))


def _one(gates, excluded=(None,), min_radius=500.0, beam_factor=0.0, **kw):
    g = np.array(gates, dtype=np.float32).reshape(-1, 3)
    ch = oracle.closest_gate_choice(g[:, 0], g[:, 1], g[:, 2], list(excluded), min_radius=min_radius, beam_factor=beam_factor,
                                    **ONE, **kw)
    return {k: (v[:, 0, 0, 0] if v.ndim == 4 else v[0, 0, 0]) for k, v in ch.items()}


def test_empty_and_out_of_reach():
    ch = _one(np.zeros((0, 3)))
    assert ch["idx32"][0] == -1 and ch["idx64"][0] == -1 and ch["n_members"] == 0 and ch["n_tied"][0] == 0
    assert np.isinf(ch["d2_win64"][0]) and np.isinf(ch["d2_min64"][0]) and np.isinf(ch["d2_second64"][0])
    ch = _one([(600.0, 0.0, 1000.0)])
    assert ch["idx32"][0] == -1 and ch["n_members"] == 0


def test_one_gate_and_the_nearer_of_two():
    ch = _one([(30.0, 40.0, 1000.0)])
    assert ch["idx32"][0] == 0 and ch["d2_win64"][0] == 2500.0 and ch["n_tied"][0] == 1 and np.isinf(ch["d2_second64"][0])
    ch = _one([(300.0, 0.0, 1000.0), (30.0, 40.0, 1000.0), (0.0, 0.0, 1400.0)])
    assert ch["idx32"][0] == 1 and ch["idx64"][0] == 1 and ch["n_members"] == 3
    assert ch["d2_min64"][0] == 2500.0 and ch["d2_second64"][0] == 90000.0


def test_tie_goes_to_the_lower_index_and_masks_are_per_field():
    gates = [(0.0, 0.0, 1400.0), (-100.0, 0.0, 1000.0), (0.0, 100.0, 1000.0), (0.0, 0.0, 900.0), (0.0, 0.0, 1000.0)]
    none = np.zeros(5, dtype=bool)
    excl = [None, none | (np.arange(5) == 4), np.isin(np.arange(5), (1, 4)), np.isin(np.arange(5), (1, 2, 3, 4)),
            np.ones(5, dtype=bool)]
    ch = _one(gates, excl)
    np.testing.assert_array_equal(ch["idx32"], [4, 1, 2, 0, -1])          # the centre gate; the three-way tie; ...
    np.testing.assert_array_equal(ch["idx64"], [4, 1, 2, 0, -1])
    np.testing.assert_array_equal(ch["n_tied"], [1, 3, 2, 1, 0])
    np.testing.assert_array_equal(ch["d2_win64"], [0.0, 1e4, 1e4, 1.6e5, np.inf])
    np.testing.assert_array_equal(ch["d2_second64"], [1e4, 1e4, 1e4, np.inf, np.inf])
    assert ch["n_members"] == 5


def test_float32_order_decides_not_float64():
    """Two gates whose float32 d2 is equal although their float64 d2 differs (found by walking the float32 lattice): the
    lower index wins in float32, the truly nearer one in float64, and the bound holds between them."""
    vx, vy, vz = 0.0, 0.0, 1000.0
    base = np.array([123.456, -77.7, 1210.9], dtype=np.float32)
    cand = roi_rim._lattice(base, 6)
    d2f = roi_rim.d2f_kernel(cand[:, 0], cand[:, 1], cand[:, 2], vx, vy, vz)
    d2 = roi_rim.d2_f64(cand[:, 0], cand[:, 1], cand[:, 2], vx, vy, vz)
    pair = None
    for v in np.unique(d2f):
        same = np.nonzero(d2f == v)[0]
        if same.size >= 2 and d2[same].max() > d2[same].min():
            far, near = same[np.argmax(d2[same])], same[np.argmin(d2[same])]
            pair = (cand[far], cand[near])
            break
    assert pair is not None
    ch = _one([pair[0], pair[1]])
    assert ch["idx32"][0] == 0 and ch["idx64"][0] == 1 and ch["n_tied"][0] == 2
    assert ch["d2_min64"][0] < ch["d2_win64"][0] <= ch["d2_min64"][0] * oracle.CLOSEST_D2_BOUND


def test_rim_membership_is_the_float64_one():
    """d2 == r2 exactly (case D) is outside; a case-A gate (float64 inside, float32 d2 >= float32 r2) is a member and wins
    when it stands alone; a case-C gate (float32 alone would admit it) is not."""
    ch = _one([(300.0, 400.0, 1000.0)])                   # 300^2 + 400^2 = 500^2
    assert ch["idx32"][0] == -1 and ch["n_members"] == 0
    rim = roi_rim.voxel_rim(0.0, 0.0, 1000.0, 500.0, 0.0)
    rng = np.random.default_rng(3)
    a = roi_rim.plant(rim, "A", rng)
    c = roi_rim.plant(rim, "C", rng)
    assert a is not None and c is not None
    assert _one([a])["idx32"][0] == 0
    ch = _one([c, a])
    assert ch["idx32"][0] == 1 and ch["n_members"] == 1 and ch["n_tied"][0] == 1
    # beam-dominated radius: r = 0.5 * |v| = 500 m, same verdicts
    assert _one([(300.0, 400.0, 1000.0)], min_radius=10.0, beam_factor=0.5)["idx32"][0] == -1
    assert _one([(299.0, 400.0, 1000.0)], min_radius=10.0, beam_factor=0.5)["idx32"][0] == 0


def test_toa_cut_altitude_and_non_finite_coordinates():
    alt = 250.0
    gates = [(10.0, 0.0, 1000.0 + alt), (50.0, 0.0, 1100.0 + alt), (np.nan, 0.0, 1000.0 + alt), (0.0, np.inf, 1000.0 + alt),
             (0.0, 0.0, np.nan), (80.0, 0.0, 950.0 + alt)]
    ch = _one(gates, radar_altitude=alt)
    assert ch["idx32"][0] == 0 and ch["n_members"] == 3                  # z is taken relative to the radar
    ch = _one(gates, radar_altitude=alt, toa=1050.0)                     # gate 1 (z_rel 1100) is cut
    assert ch["idx32"][0] == 0 and ch["n_members"] == 2
    ch = _one(gates, radar_altitude=alt, toa=999.0)                      # gates 0 and 1 are cut: gate 5 is left
    assert ch["idx32"][0] == 5 and ch["n_members"] == 1
    ch = _one(gates, radar_altitude=alt, toa=1000.0)                     # z_rel == toa is kept (compute.py:193)
    assert ch["idx32"][0] == 0


def test_cache_returns_the_first_result():
    g = np.array([[10.0, 0.0, 1000.0]], dtype=np.float32)
    a = oracle.closest_gate_choice(g[:, 0], g[:, 1], g[:, 2], [None], min_radius=500.0, beam_factor=0.0, cache_key="t", **ONE)
    b = oracle.closest_gate_choice(g[:, 0], g[:, 1], g[:, 2], [None], min_radius=500.0, beam_factor=0.0, cache_key="t", **ONE)
    assert a is b


def test_agrees_with_closest_gate_grid_where_its_gap_is_clear():
    """The cloud of tests/test_gpu_edges.py::test_closest_gate_mode_and_processor_seam_package: wherever the older oracle's
    two nearest gates are more than 1e-2 m^2 apart both pick the same gate, and the filled voxels are the same everywhere."""
    from radar_processor_amd import processor_seam as seam
    rng = np.random.default_rng(12)
    n = 60 * 80
    gx = rng.uniform(-9e3, 9e3, n).astype(np.float32)
    gy = rng.uniform(-9e3, 9e3, n).astype(np.float32)
    gz = rng.uniform(0, 3e3, n).astype(np.float32)
    drop = rng.random(n) < 0.25
    zl, yl, xl, res = (0.0, 2400.0), (-8000.0, 8000.0), (-6000.0, 6000.0), 400.0
    shape, roi = seam.grid3d_shape(zl, yl, xl, res), seam.constant_roi_for(res, yl)
    values = np.arange(n, dtype=np.float32)
    want, gap = oracle.closest_gate_grid(gx, gy, gz, values, drop, shape, (zl, yl, xl), roi)
    ch = oracle.closest_gate_choice(gx, gy, gz, [drop], shape, (zl, yl, xl), roi, 0.0)
    idx = ch["idx32"][0]
    np.testing.assert_array_equal(idx < 0, np.isnan(want))
    clear = (gap > 1e-2) & (idx >= 0)
    assert clear.mean() > 0.5
    np.testing.assert_array_equal(idx[clear], want[clear].astype(np.int64))
    np.testing.assert_array_equal(ch["idx64"][0][idx >= 0], want[idx >= 0].astype(np.int64))   # both are float64 argmins


# ---- the scenes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cs.SCENES)
def test_float64_bound_on_every_filled_voxel(name):
    """d2_win64 <= d2_min64 (1 + 5u) / (1 - 5u): the float32 winner is, to float64, as near as the nearest live member up to
    the derived rounding bound -- in every field (each has its own mask) and with the shared mask."""
    s = cs.scene(name)
    for ch in (s.choice(), s.choice_shared()):
        filled = ch["idx32"] >= 0
        np.testing.assert_array_equal(filled, ch["idx64"] >= 0)
        np.testing.assert_array_equal(filled, np.isfinite(ch["d2_min64"]))
        assert np.all(ch["d2_win64"][filled] >= ch["d2_min64"][filled])
        assert np.all(ch["d2_win64"][filled] <= ch["d2_min64"][filled] * oracle.CLOSEST_D2_BOUND)
        same = filled & (ch["idx32"] == ch["idx64"])
        np.testing.assert_array_equal(ch["d2_win64"][same], ch["d2_min64"][same])
        assert np.all(ch["n_tied"][filled] >= 1) and np.all(ch["n_tied"][~filled] == 0)
        # no squares in the subnormal range: a winner is exactly on the voxel centre or well away from it
        pos = ch["d2_min64"][filled]
        assert np.all((pos == 0) | (pos > 1e-6))
    print(name, cs.summary(s))


@pytest.mark.parametrize("name", ["polar_const", "polar_beam", "ragged_a", "ragged_b"])
def test_filled_share(name):
    s = cs.scene(name)
    filled = s.choice()["idx32"] >= 0
    for f in range(cs.N_MASKS):
        assert 0.3 <= filled[f].mean() <= 0.95, (name, f, filled[f].mean())
    assert s.n_gates < 2 ** 24                                            # index-coded values are exact


def test_masks_differ_per_field_and_change_the_winner():
    for name in cs.SCENES:
        s = cs.scene(name)
        masks = s.masks()
        assert [m is None for m in masks] == [bool(k % 2) for k in range(cs.N_MASKS)]
        even = [m for m in masks if m is not None]
        assert all(m.shape == (s.n_gates,) and m.dtype == bool for m in even)
        assert all(not np.array_equal(a, b) for i, a in enumerate(even) for b in even[i + 1:])
        idx, n_tied = s.choice()["idx32"], s.choice()["n_tied"]
        for k in range(0, cs.N_MASKS, 2):
            # the mask changes winners (the ties scene's field 2 removes tied losers only: it changes the tie counts)
            assert ((idx[k] != idx[1]) | (n_tied[k] != n_tied[1])).sum() >= 10, (name, k)
            filled = idx[k] >= 0
            assert not masks[k][idx[k][filled]].any()
        np.testing.assert_array_equal(idx[1], idx[3])
        sh = s.choice_shared()["idx32"]
        assert (sh[1] != idx[1]).sum() >= 10 and not s.shared_mask()[sh[1][sh[1] >= 0]].any()


def test_polar_const_has_natural_float32_ties_and_is_the_seams_grid():
    from radar_processor_amd import processor_seam as seam
    s = cs.scene("polar_const")
    assert s.shape == (5, 23, 37) and s.min_radius == seam.constant_roi_for(cs.POLAR_RES, cs.POLAR_Y) == 1500.0
    zc, yc, xc = roi_rim.voxel_centres(s.shape, s.limits)
    assert np.array_equal(xc, -xc[::-1]) and np.array_equal(yc, -yc[::-1])     # centred on the radar
    ch = s.choice()
    assert (ch["n_tied"][1] > 1).sum() >= 1                                     # with nothing excluded ...
    assert sum(int((ch["n_tied"][k] > 1).sum()) for k in range(0, cs.N_MASKS, 2)) >= 1     # ... and under a mask


def test_polar_beam_roi_grows_and_toa_cuts():
    s = cs.scene("polar_beam")
    zc, yc, xc = roi_rim.voxel_centres(s.shape, s.limits)
    r = [np.sqrt(roi_rim.voxel_rim(x, y, z, s.min_radius, s.beam_factor).r2) for x, y, z in
         ((xc[np.argmin(np.abs(xc))], yc[np.argmin(np.abs(yc))], zc[0]), (xc[0], yc[0], zc[-1]))]
    assert r[0] < 200.0 and r[1] > 1200.0 and s.radar_altitude != 0.0 and np.isfinite(s.toa)
    z_rel = s.gz - F32(s.radar_altitude)
    assert 100 < np.count_nonzero(z_rel > F32(s.toa)) < s.n_gates // 2
    uncut = oracle.closest_gate_choice(s.gx, s.gy, s.gz, [None], s.shape, s.limits, s.min_radius, s.beam_factor,
                                       radar_altitude=s.radar_altitude)["idx32"][0]
    assert (uncut != s.choice()["idx32"][1]).sum() >= 10                        # the cut changes winners


@pytest.mark.parametrize("name", ["ragged_a", "ragged_b"])
def test_ragged_cloud_overflows_the_survivor_ring(name):
    """A voxel's members all survive its block's pre-filter, so a voxel with more than 256 members means a block that queues
    more than the 256 slots of the ring (several times over here), on a grid ragged against the 16 x 4 patch."""
    s = cs.scene(name)
    nz, ny, nx = s.shape
    assert nx % 16 and ny % 4 and nx % 4
    members = s.choice()["n_members"]
    assert members.max() > 600 and (members > 256).mean() > 0.2, (members.max(), (members > 256).mean())
    ragged = members[:, ny - ny % 4:, nx - nx % 4:]                             # the corner block: 1-3 voxels wide and high
    assert ragged.max() > 256 or name == "ragged_a"
    assert members[:, ny - ny % 4:, :].max() > 256                              # a ragged row of blocks overflows too


def test_planted_ties_are_present_with_their_labels():
    s = cs.scene("ties")
    ch = s.choice()
    idx, n_tied = ch["idx32"].reshape(cs.N_MASKS, -1), ch["n_tied"].reshape(cs.N_MASKS, -1)
    kinds = {t.kind for t in s.ties}
    assert kinds == set(cs.TIE_KINDS) | {"far"} and len(s.ties) == s.n_vox
    assert sum(t.kind == "far" for t in s.ties) == len(cs.TIES_FAR_VOXELS)
    for t in s.ties:
        v, tied = t.voxel, t.tied
        assert list(tied) == sorted(tied)
        assert idx[1, v] == tied[0] and n_tied[1, v] == len(tied), t       # nothing excluded: the lowest index of the tie
        assert idx[3, v] == tied[0]
        if t.kind == "centre":
            assert ch["d2_win64"][1].ravel()[v] == 0.0
            assert idx[0, v] == t.other and idx[2, v] == tied[0]             # the runner-up once the centre gate is excluded
            continue
        # the lower index excluded for field 0 and live for fields 1-3; the highest excluded for field 2
        assert idx[0, v] == tied[1] and n_tied[0, v] == len(tied) - 1, t
        assert idx[2, v] == tied[0] and n_tied[2, v] == len(tied) - 1, t
        if len(tied) == 3:
            assert idx[4, v] == tied[2] and n_tied[4, v] == 1, t
        else:
            assert idx[4, v] == tied[0] and n_tied[4, v] == 2, t
        g = np.array(tied)
        same_place = np.all(s.gx[g] == s.gx[g[0]]) and np.all(s.gy[g] == s.gy[g[0]]) and np.all(s.gz[g] == s.gz[g[0]])
        assert same_place == (t.kind in ("dup", "dup_centre"))
        if t.kind == "dup_centre":
            assert ch["d2_win64"][1].ravel()[v] == 0.0
        if t.kind == "mirror_y":
            assert s.gy[tied[0]] > s.gy[tied[1]]                             # the lower index lies in the later cell row
        if t.kind == "far":
            # more than 256 other members of the voxel between the tied gates, by index and by y (the two orders a cell
            # list can have), and the lower index on the side the scene names
            side = cs.TIES_FAR_VOXELS[v]
            assert np.sign(s.gy[tied[0]] - s.gy[tied[1]]) == side
            lo_y, hi_y = sorted((s.gy[tied[0]], s.gy[tied[1]]))
            between = (np.arange(s.n_gates) > tied[0]) & (np.arange(s.n_gates) < tied[1]) & (s.gy > lo_y) & (s.gy < hi_y)
            zc, yc, xc = roi_rim.voxel_centres(s.shape, s.limits)
            iz, rem = divmod(v, s.shape[1] * s.shape[2]); iy, ix = divmod(rem, s.shape[2])
            near = roi_rim.d2_f64(s.gx, s.gy, s.gz, float(xc[ix]), float(yc[iy]), float(zc[iz])) < s.min_radius ** 2
            assert np.count_nonzero(between & near) > 256 and ch["n_members"].ravel()[v] > 258
    sides = set(cs.TIES_FAR_VOXELS.values())
    assert sides == {1, -1}


def test_rim_scene_covers_every_case():
    s = cs.scene("rim")
    lab = cs.rim_labels(s)
    counts = {c: int(np.count_nonzero(lab == c)) for c in roi_rim.CASES}
    print("rim cases:", counts)
    assert all(counts[c] >= 20 for c in roi_rim.CASES), counts
    ch = s.choice()
    idx, members = ch["idx32"][1].ravel(), ch["n_members"].ravel()
    # A and B are members of their voxel, C and D are not
    vox_of = s.rim_voxel
    zc, yc, xc = roi_rim.voxel_centres(s.shape, s.limits)
    iz, rem = np.divmod(vox_of, s.shape[1] * s.shape[2]); iy, ix = np.divmod(rem, s.shape[2])
    inside = roi_rim.d2_f64(s.gx, s.gy, s.gz, xc[ix].astype(np.float64), yc[iy].astype(np.float64),
                            zc[iz].astype(np.float64)) < s.min_radius ** 2
    assert inside[np.isin(lab, ["A", "B"])].all() and not inside[np.isin(lab, ["C", "D"])].any()
    # voxels whose ONLY member is a case-A gate: it wins; voxels whose only planted gates are outside: empty
    alone_a = [g for g in np.nonzero(lab == "A")[0] if members[vox_of[g]] == 1]
    assert len(alone_a) >= 10 and all(idx[vox_of[g]] == g for g in alone_a)
    planted = np.bincount(vox_of, minlength=s.n_vox)
    assert np.count_nonzero((planted > 0) & (members == 0)) >= 10
    np.testing.assert_array_equal(members, np.bincount(vox_of[inside], minlength=s.n_vox))   # a gate reaches its own voxel only
    assert 0 < (idx >= 0).mean() < 1


def test_real_values_plant_specials_on_winners():
    for name in cs.SCENES:
        s = cs.scene(name)
        val, special = s.real_values()
        assert len(set(special.values())) == 5
        won = s.choice()["idx32"][1]
        assert all((won == g).any() for g in special.values())
        assert np.signbit(val[special["neg_zero"]]) and val[special["neg_zero"]] == 0
        assert 0 < val[special["subnormal"]] < np.finfo(np.float32).tiny
        assert np.isposinf(val[special["pos_inf"]]) and np.isneginf(val[special["neg_inf"]]) and np.isnan(val[special["nan"]])


def test_recorded_scene_numbers_are_current():
    """profiles/closest_bounds.json holds what the scenes give now (reference-side numbers only)."""
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "closest_bounds.json")
    with open(path) as f:
        rec = json.load(f)["scenes"]
    assert sorted(rec) == sorted(cs.SCENES)
    for name in cs.SCENES:
        now = cs.summary(cs.scene(name))
        assert sorted(rec[name]) == sorted(now)
        for key, v in now.items():
            assert rec[name][key] == pytest.approx(v, rel=1e-9, abs=1e-15), (name, key)
        assert now["worst_d2_ratio_minus_1"] <= now["bound_minus_1"]
