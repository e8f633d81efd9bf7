"""CPU checks that every scene of tests/shear_scenes.py contains what it is there for (no GPU needed)."""
import numpy as np

import shear_oracle as so
import shear_scenes as ss


def _moments(name):
    s = ss.scenes()[name]
    return so.moments(s["vel"], s["mask"], s["half_rays"], s["max_half_rays"], s["half_gates"], s["wrap"])


def _defined(name):
    return ~np.isnan(ss.reference(name).az_shear)


def test_seams():
    wrap, open_ = ss.scenes()["seams_wrap"], ss.scenes()["seams_open"]
    assert wrap["vel"].shape == (2, 37, 150) and wrap["half_gates"] == 3 and wrap["max_half_rays"] == 16
    assert set(wrap["half_rays"].tolist()) == {0, 1, 2, 5, 16, 40} and wrap["wrap"] == 1 and open_["wrap"] == 0
    for tile in range(0, 150, 32):                                 # half-widths change inside every 32 gates
        assert len(set(wrap["half_rays"][tile:tile + 32].tolist())) >= 3
    ok = so.valid(wrap["vel"], wrap["mask"])
    assert 0.22 < 1.0 - ok.mean() < 0.35 and np.isnan(wrap["vel"]).any() and wrap["mask"].any()
    assert not np.array_equal(so.bits(wrap["vel"][0]), so.bits(wrap["vel"][1]))
    a, b = ss.reference("seams_wrap"), ss.reference("seams_open")
    # the wrap changes ray 0 and ray 36, and only rays within 16 of the seam
    differ = (so.bits(a.az_shear) != so.bits(b.az_shear)) | (a.count != b.count)
    assert differ[:, 0].any() and differ[:, 36].any() and not differ[:, 16:21].any()
    # a gate whose half-width is 40 counts as 16: its window is 33 rays, the whole circle but four
    wide = wrap["half_rays"] == 40
    assert a.count[:, :, wide].max() > 29 * 7 * 0.6
    assert _defined("seams_wrap").any() and not _defined("seams_wrap")[:, :, wrap["half_rays"] == 0].any()
    # leaking into the other sweep would change the result: the sweeps' results differ
    assert not np.array_equal(a.count[0], a.count[1])


def test_full_circle():
    s = ss.scenes()["full_circle"]
    assert s["vel"].shape[1] == 33 == 2 * 16 + 1 and s["wrap"] == 1 and set(s["half_rays"].tolist()) == {16}
    count = ss.reference("full_circle").count
    assert (count == count[:, :1]).all()                          # every ray sees the same set of gates
    assert _defined("full_circle").any()


def test_small_shapes():
    for name in ("one_ray", "two_rays", "one_gate", "five_gates"):
        assert ss.reference(name).count.max() > 0, name
    m, _ = _moments("one_ray")
    A = so.normal_terms(m)[0]
    assert (A == 0).all() and not _defined("one_ray").any()
    m, _ = _moments("one_gate")
    assert (so.normal_terms(m)[2] == 0).all() and not _defined("one_gate").any()
    s = ss.scenes()["five_gates"]
    assert s["vel"].shape[2] == 5 < s["half_gates"]
    assert ss.scenes()["two_rays"]["vel"].shape[1] == 2


def test_degenerate_windows_have_a_zero_determinant():
    for name in ("degenerate_single_ray", "degenerate_single_column", "degenerate_diagonal"):
        m, _ = _moments(name)
        D = so.normal_terms(m)[5]
        assert (D == 0).all(), name
        assert (m["n"] >= ss.scenes()[name]["min_valid"]).any(), name     # only D = 0 keeps these gates undefined
        ref = ss.reference(name)
        for plane in ref[:3]:
            assert (so.bits(plane) == so.NAN_BITS).all(), name


def test_magnitudes_reach_the_bound_of_p():
    s = ss.scenes()["magnitudes"]
    m, ok = _moments("magnitudes")
    P = so.normal_terms(m)[3]
    largest = max(abs(int(v)) for v in P.reshape(-1).tolist())
    # the same in Python ints at the gate where it is largest: int64 did not wrap
    at = np.unravel_index(np.argmax(np.abs(P)), P.shape)
    exact = {k: int(v[at]) for k, v in m.items()}
    assert exact["n"] * exact["Siq"] - exact["Si"] * exact["Sq"] == int(P[at])
    assert 2 ** 53 < largest < 2 ** 56 and at[0] == 0
    # the checkerboard along i: (-1)^i is even in i, so sum(i * q) over a full circle of offsets cancels EXACTLY and P = 0
    assert (P[1] == 0).all() and (np.abs(s["vel"][1]) == 16384.0).all() and (np.abs(m["Sq"][1]) > 2 ** 34).any()
    assert (np.diff(np.sign(s["vel"][1, :, 0])) != 0).all()
    assert exact["n"] == 1089
    assert not ok[0, 50, 2] and not ok[0, 51, 3] and ok.sum() == ok.size - 2
    assert s["vel"][0, 50, 2] > 16384.0 and np.isinf(s["vel"][0, 51, 3])
    assert np.isfinite(ss.reference("magnitudes").az_shear[at])


def test_plane_is_exact_in_fixed_point():
    s = ss.scenes()["plane"]
    q = np.rint(s["vel"].astype(np.float64) * 65536.0)
    assert np.array_equal(q / 65536.0, s["vel"].astype(np.float64))
    a, g = np.meshgrid(np.arange(50), np.arange(70), indexing="ij")
    assert np.array_equal(q[0], ss.PLANE["c0"] + ss.PLANE["c1"] * a + ss.PLANE["c2"] * g)
    m, ok = _moments("plane")
    assert ok.all()
    inside = ss.interior("plane")
    assert inside.any() and not inside.all()
    A, B, C, P, Q, D = so.normal_terms(m)
    assert (B[inside] == 0).all() and (m["Si"][inside] == 0).all() and (m["Sj"][inside] == 0).all()
    assert (P[inside] == ss.PLANE["c1"] * A[inside]).all() and (Q[inside] == ss.PLANE["c2"] * C[inside]).all()


def test_each_threshold_flips_gates():
    base = _defined("thresholds_base")
    flipped = {name: int((base & ~_defined("thresholds_" + name)).sum()) for name in ("min_valid", "fraction", "centre")}
    assert all(count >= 1 for count in flipped.values()), flipped
    for name in flipped:
        assert _defined("thresholds_" + name).any(), name             # and none of them empties the scene
        assert not (~base & _defined("thresholds_" + name)).any()
        assert np.array_equal(ss.reference("thresholds_" + name).count, ss.reference("thresholds_base").count)


def test_bands_span_several_workgroups():
    s = ss.scenes()["bands_wrap"]
    assert s["vel"].shape == (2, 95, 70) and s["half_gates"] == 16 and {0, 16} <= set(s["half_rays"].tolist())
    assert _defined("bands_wrap").any() and _defined("bands_open").any() and _defined("bands_narrow").any()
    assert ss.scenes()["bands_narrow"]["max_half_rays"] == 2 and ss.scenes()["bands_narrow"]["half_rays"].max() == 2


def test_median_data_holds_ties_holes_and_both_parities():
    vel, mask = ss.median_data()
    ok = so.valid(vel, mask)
    assert np.isnan(vel).any() and np.isinf(vel).any() and mask.any() and not (vel == 0).any()
    values = vel[ok]
    assert len(np.unique(values)) < values.size // 4                 # ties
    window = sum(np.roll(np.roll(ok, i, 1), j, 2).astype(int) for i in (-1, 0, 1) for j in (-1, 0, 1))
    assert (window % 2 == 0).any() and (window % 2 == 1).any()
    cases = ss.median_cases()
    assert {(c[0], c[1]) for c in cases} == {(a, b) for a in range(3) for b in range(3)} - {(0, 0)}
    assert {c[2] for c in cases} == {0, 1} and {c[4] for c in cases} == {0, 1} and {c[3] for c in cases} == {1, 4}
    # wrap across ray 0 and centre_only change the result
    a = so.median(vel, mask, 1, 1, 1, 1, 1)
    assert not np.array_equal(so.bits(a[:, 0]), so.bits(so.median(vel, mask, 1, 1, 0, 1, 1)[:, 0]))
    assert not np.array_equal(so.bits(a), so.bits(so.median(vel, mask, 1, 1, 1, 1, 0)))
    assert not np.array_equal(so.bits(a), so.bits(so.median(vel, mask, 1, 1, 1, 4, 1)))
