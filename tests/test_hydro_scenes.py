"""The frozen scenes of tests/hydro_scenes.py hold what they are said to hold (no GPU needed): asserted through the NumPy
restatement alone, so that a GPU test that passes on them has met the cases by construction and not by luck."""
import numpy as np
import pytest

import hydro_oracle as ho
import hydro_scenes as hs


# ---- texture -----------------------------------------------------------------------------------------------------------------
def test_texture_shapes_straddle_the_tile_and_every_array_is_frozen():
    scenes = hs.texture_scenes()
    T = hs.TILE
    shapes = {(s["x"].shape[1], s["x"].shape[0], s["half_gates"]) for name, s in scenes.items() if name.startswith("shape_")}
    for G in (1, 2, 64, 65, 126, 127, 128, 513, T - 1, T, T + 1, T + 63, T + 64):
        for R in (1, 3, 5):
            for L in (1, 2, 63):
                assert (G, R, L) in shapes
    for s in scenes.values():
        assert s["x"].dtype == np.float32 and not s["x"].flags.writeable
        assert s["mask"] is None or (s["mask"].dtype == np.uint8 and not s["mask"].flags.writeable)
        assert 1 <= s["half_gates"] <= 63 and 1 <= s["min_valid"] <= 127
    assert {s["centre_only"] for s in scenes.values()} == {0, 1}
    assert any(s["mask"] is None for s in scenes.values()) and any(s["mask"] is not None for s in scenes.values())


def test_texture_scenes_hold_their_cases():
    scenes = hs.texture_scenes()
    ref = hs.texture_reference("holes_mask")
    s = scenes["holes_mask"]
    assert np.isnan(s["x"]).mean() > 0.2 and (s["mask"] != 0).mean() > 0.1
    assert 0.1 < np.isnan(ref.sd).mean() < 0.9 and ref.count.min() < s["min_valid"] <= ref.count.max()
    # a ray with no valid gate: count 0 and NaN along the whole ray, whatever min_valid
    ref = hs.texture_reference("empty_rays")
    for ray in (1, 2):
        assert (ref.count[ray] == 0).all() and (ho.bits(ref.sd[ray]) == ho.NAN_BITS).all() and (ho.bits(ref.mean[ray]) == ho.NAN_BITS).all()
    assert (ref.count[0] > 0).any() and not np.isnan(ref.sd[3]).all()
    # +-8192 is valid, the next float32 beyond is not
    s, ref = scenes["limits"], hs.texture_reference("limits")
    ok = ho.valid(s["x"])
    assert ok[0].all() and ok[1, 55] and ok[1, 56] and not ok[1, [50, 51, 52, 53, 54, 57, 58, 59]].any()
    assert ref.count.max() == 127 and abs(float(ref.sd[0, 100]) - 8192.0 * np.sqrt(1.0 - 1.0 / 127 ** 2)) < 1e-3      # alternating +-8192
    q = ho.fixed(s["x"], ok)
    assert int(np.abs(q).max()) == 2 ** 23
    window = q[0, 37:164].astype(object)                                  # the full window of gate 100: the largest sums there are
    assert 127 * int((window * window).sum()) == 127 * 127 * 2 ** 46 < 2 ** 60
    # a constant ray: D == 0, sd == +0.0 exactly, the mean is the value to 2^-10
    ref = hs.texture_reference("constant")
    assert (ho.bits(ref.sd) == 0).all()
    assert (ref.mean[0] == np.float32(np.rint(3.7 * 1024) / 1024)).all() and (ref.mean[1] == np.float32(-8192.0)).all()
    # min_valid at N and at N + 1
    at, above = hs.texture_reference("min_valid_at_n"), hs.texture_reference("min_valid_above_n")
    assert (at.count[:, 3:-3] == 7).all() and at.count.max() == 7
    assert not np.isnan(at.sd[:, 3:-3]).any() and np.isnan(at.sd[:, :3]).all() and np.isnan(at.sd[:, -3:]).all()
    assert np.isnan(above.sd).all() and np.array_equal(above.count, at.count)
    # more tiles than workgroups
    s = scenes["many_rays"]
    assert s["x"].shape[0] * -(-s["x"].shape[1] // hs.TILE) > 1 << 20


def test_every_texture_reference_is_defined_somewhere_and_missing_somewhere_overall():
    defined = missing = 0
    for name in hs.texture_scenes():
        ref = hs.texture_reference(name)
        assert ref.sd.dtype == np.float32 and ref.mean.dtype == np.float32 and ref.count.dtype == np.uint16
        nan = np.isnan(ref.sd)
        assert np.array_equal(nan, np.isnan(ref.mean)) and (ho.bits(ref.sd)[nan] == ho.NAN_BITS).all()
        assert (ref.sd[~nan] >= 0).all()
        defined += int((~nan).sum())
        missing += int(nan.sum())
    assert defined > 1000 and missing > 1000


# ---- classifier --------------------------------------------------------------------------------------------------------------
def test_classifier_shapes():
    scenes = hs.classifier_scenes()
    assert {(s["B"], s["C"], s["V"]) for s in scenes.values()} >= {(1, 1, 1), (2, 2, 3), (32, 4, 8), (8, 16, 8)}
    assert {s["S"] for s in scenes.values()} == {1, 3}
    assert any(s["B"] * s["C"] * s["V"] == 1024 for s in scenes.values())
    for name, s in scenes.items():
        assert s["spec"].cells.shape == (s["B"], s["C"], s["V"], 6) and s["spec"].weights.shape == (s["C"], s["V"])
        assert len(s["spec"].edges) == s["B"] - 1 and all(b > a for a, b in zip(s["spec"].edges, s["spec"].edges[1:]))
        assert 0 in s["spec"].kinds and (s["V"] < 3 or 1 in s["spec"].kinds)
        for v, a in enumerate(s["fields"]):
            rows = s["S"] if (s["per_sweep_bits"] >> v) & 1 else s["R"]
            assert a.dtype == np.float32 and a.shape == (rows, s["G"]) and not a.flags.writeable, (name, v)
        assert s["V"] < 3 or s["per_sweep_bits"] != 0
        assert s["rays_per_sweep"] * s["S"] == s["R"]
    # the classifier launches as many workgroups as the device holds at once: three per CU under a 48 KB table, on the 256 CUs of
    # the whole part (a partition has fewer, which only lowers the number of gates from which the workgroups stride)
    assert scenes["strides"]["B"] * scenes["strides"]["C"] * scenes["strides"]["V"] * 48 > 160 * 1024 // 4
    assert scenes["strides"]["R"] * scenes["strides"]["G"] > 3 * 256 * 256


@pytest.mark.parametrize("name", sorted(hs.CLASSIFIER_SHAPES) + ["strides"])
def test_classifier_scene_conditions(name):
    s, ref = hs.classifier_scenes()[name], hs.classifier_reference(name)
    wins = np.bincount(ref.cls.reshape(-1), minlength=s["C"] + 1)
    assert (wins[1:] > 0).all(), f"{name}: a class never wins: {wins.tolist()}"
    unclassified = (ref.cls == 0).mean()
    assert 0.05 <= unclassified <= 0.60, f"{name}: {unclassified:.3f} of the gates are unclassified"
    assert ((ref.second != ref.cls) | (ref.second == 0)).all()
    assert (ref.second[ref.cls == 0] == 0).all() and (ho.bits(ref.score)[ref.cls == 0] == ho.NAN_BITS).all()
    assert (ref.score[ref.cls != 0] > 0).all() and (ref.second.max() <= s["C"])
    if s["C"] == 1:
        assert (ref.second == 0).all()
    else:
        assert (ref.second[ref.cls != 0] != 0).all()
    if s["B"] > 1:                                                        # every bin occurs among the classified gates
        full = ho.expand(s["fields"], s["per_sweep_bits"], s["rays_per_sweep"])
        cond = full[s["spec"].cond_var]
        with np.errstate(invalid="ignore"):
            bins = sum((cond >= np.float32(e)).astype(int) for e in s["spec"].edges)
        assert set(np.unique(bins[ref.cls != 0]).tolist()) == set(range(s["B"])), name
        # values exactly ON every edge, and one float32 below
        for e in s["spec"].edges:
            assert (cond == np.float32(e)).any() and (cond == np.nextafter(np.float32(e), np.float32(-np.inf))).any()


@pytest.mark.parametrize("name", sorted(hs.classifier_scenes()))
def test_every_finite_vertex_of_every_cell_is_met_by_a_scored_gate_of_its_own_bin(name):
    """Every (bin, class, variable, vertex) that is finite, of every variable but the condition variable -- per-sweep variable
    included -- is the value of that variable at a gate that is not masked, misses nothing required, gets scores, and lies in the
    bin where that cell is read."""
    s = hs.classifier_scenes()[name]
    met, there = hs.vertices_met(s, hs.classifier_reference(name))
    expected = int(np.isfinite(np.delete(s["vertices"], s["spec"].cond_var, axis=2) if s["spec"].cond_var >= 0 else s["vertices"]).sum())
    assert there == expected and there >= (4 if s["V"] == 1 else 12)
    assert met == there, f"{name}: only {met} of {there} finite vertices are met"


@pytest.mark.parametrize("name", ["small", "bins32_sweeps", "cap1024"])
def test_ties_are_planted(name):
    s, ref = hs.classifier_scenes()[name], hs.classifier_reference(name)
    full = ho.expand(s["fields"], s["per_sweep_bits"], s["rays_per_sweep"])
    # the last two classes are the same in bin 0: wherever one of them wins there the other is the runner-up with the SAME score,
    # and it is the lower one that wins
    C = s["C"]
    with np.errstate(invalid="ignore"):
        bin0 = full[s["spec"].cond_var] < np.float32(s["spec"].edges[0])
    tie = bin0 & (ref.cls == C - 1)
    assert tie.sum() >= 3 and (ref.second[tie] == C).all() and not (bin0 & (ref.cls == C)).any()
    one = hs.tiny(dict(s, fields=[a for a in s["fields"]]), 1, s["G"])
    flat = np.flatnonzero(tie[0])[:2]
    if len(flat):
        cut = dict(one, fields=[np.ascontiguousarray(a[:, flat]) for a in one["fields"]], mask=np.ascontiguousarray(one["mask"][:, flat]))
        naive = ho.classify_naive(*hs.classifier_args(cut))
        assert (naive.cls == C - 1).all() and (naive.second == C).all()


def test_missing_variables_of_every_kind_occur():
    for name in ("bins32", "cap1024"):
        s, ref = hs.classifier_scenes()[name], hs.classifier_reference(name)
        full = ho.expand(s["fields"], s["per_sweep_bits"], s["rays_per_sweep"])
        spec = s["spec"]
        required = [v for v in range(s["V"]) if (spec.required_bits >> v) & 1]
        optional = [v for v in range(s["V"]) if v not in required and v != spec.cond_var]
        assert len(required) == 2
        for v in required + [spec.cond_var]:
            gone = ~np.isfinite(full[v])
            assert gone.any() and (ref.cls[gone] == 0).all(), (name, v)
        some = np.zeros(ref.cls.shape, bool)
        for v in optional:
            some |= ~np.isfinite(full[v])
        assert (some & (ref.cls != 0)).sum() > 50, name                      # a missing optional variable still classifies
        assert {float(a[~np.isfinite(a)][0]) if (~np.isfinite(a)).any() and not np.isnan(a[~np.isfinite(a)][0]) else "nan"
                for a in full} >= {"nan", float("inf"), float("-inf")}
        assert (s["mask"] != 0).any() and (ref.cls[s["mask"] != 0] == 0).all()


def test_a_class_of_all_zero_weights_never_wins_and_min_score_cuts_at_the_score():
    scenes = hs.classifier_scenes()
    s, ref = scenes["zero_weights"], hs.classifier_reference("zero_weights")
    assert (s["spec"].weights[1] == 0).all() and not (ref.cls == 2).any() and (ref.cls == 1).any() and (ref.cls == 3).any()
    assert (ref.second == 2).any()                                         # its score is 0: it can still run up
    at, pivot = scenes["min_score_at"]["pivot_gate"], scenes["min_score_at"]["pivot"]
    above, exact, below = (hs.classifier_reference(n) for n in ("min_score_above", "min_score_at", "min_score_below"))
    assert scenes["min_score_above"]["min_score"] > pivot == scenes["min_score_at"]["min_score"] > scenes["min_score_below"]["min_score"]
    assert above.cls.reshape(-1)[at] == 0 and exact.cls.reshape(-1)[at] != 0 and below.cls.reshape(-1)[at] != 0
    assert above.best.reshape(-1)[at] == pivot and (above.cls == 0).sum() > (exact.cls == 0).sum()
