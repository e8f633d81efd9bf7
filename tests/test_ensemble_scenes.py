"""The scenes of tests/ensemble_scenes.py reach what they claim -- shown on the CPU, through the oracle alone, so that the GPU
tests which compare against them cannot pass on scenes that miss their point."""
import numpy as np

import ensemble_oracle as eo
import ensemble_scenes as es


def test_the_launch_constants_were_found_in_the_sources():
    assert es.BLOCK == 256 and es.HIST_MAX_STRIPS is not None and es.HIST_MAX_STRIPS >= 1


def test_rim_has_pixels_with_no_member_with_some_and_with_all():
    s = es.rim(1)
    h, w = s.src.shape
    assert (h, w) == (37, 53) and h % 4 and w % 4 and (h * w) // es.BLOCK == 7 and (h * w) % es.BLOCK
    assert np.abs(s.shifts).max() == 60.0 and s.n_members == 5
    members = es.expected("rim-min1").members
    assert (members == 0).any() and ((members >= 1) & (members <= 4)).any() and (members == 5).any()
    assert (members[2] == 0).all()                                           # a lead without a single member anywhere
    # min_members decides where prob and mean are NaN, and nothing else
    one, five = es.expected("rim-min1"), es.expected("rim-min5")
    assert np.array_equal(one.counts, five.counts) and np.array_equal(one.members, five.members)
    assert np.array_equal(np.isnan(one.prob[:, 0]), members == 0) and np.array_equal(np.isnan(five.prob[:, 0]), members < 5)
    assert (np.isnan(five.mean) & ~np.isnan(one.mean)).any()


def test_caps_fills_all_eight_fields_with_64():
    s = es.caps()
    assert s.src.shape == (20, 70) and s.n_members == 64 and len(s.thresholds) == 8 and len(s.leads) == 16 and s.substeps == 16
    counts = es.expected("caps").counts
    full = (counts == 64).all(axis=1)                                        # [L, h, w]: every threshold at 64
    assert full.any(axis=(1, 2)).all(), "every lead has a pixel whose eight counts are all 64"
    assert (counts.max(axis=(0, 2, 3)) == 64).all() and (counts.min(axis=(0, 2, 3)) < 64).all()


def test_ties_holds_equalities_infinities_signed_zero_and_holes():
    s = es.ties()
    equal, minus_zero, infs, holes = 0, 0, 0, 0
    for l, lead in enumerate(s.leads):
        v = eo.member_samples(s.src, s.motion, s.lattice, lead, s.shifts[l], s.substeps, s.method)
        equal += int(sum((v == t).sum() for t in s.thresholds if t != 0.0))
        minus_zero += int(((v == 0.0) & np.signbit(v)).sum())
        infs += int(np.isinf(v).sum())
        holes += int(np.isnan(v).sum())
    assert equal >= 20 and minus_zero >= 5 and infs >= 10 and holes >= 10
    want = es.expected("ties")
    assert np.isnan(want.mean[want.members >= s.min_members]).any(), "inf - inf among present members: a NaN mean"
    assert np.isinf(want.mean).any()


def test_lattice_has_weight_sums_on_both_sides_of_one_half():
    s = es.lattice()
    assert s.src.shape == (70, 129) and (s.lattice.ny, s.lattice.nx) == (3, 4) and s.substeps == 3 and s.method == "bilinear"
    assert (s.shifts != np.round(s.shifts)).all()
    below = above = 0
    for l, lead in enumerate(s.leads):
        ws = eo.weight_sums(s.src, s.motion, s.lattice, lead, s.shifts[l], s.substeps)
        v = eo.member_samples(s.src, s.motion, s.lattice, lead, s.shifts[l], s.substeps, s.method)
        lo, hi = (ws > 0.0) & (ws < 0.5), (ws >= 0.5) & (ws < 1.0)
        assert np.isnan(v[lo]).all() and not np.isnan(v[hi]).any()
        below, above = below + int(lo.sum()), above + int(hi.sum())
    assert below >= 50 and above >= 50
    members = es.expected("lattice").members
    assert (members < s.min_members).any() and (members == s.n_members).any()


def test_slivers_are_the_three_shapes_in_both_methods():
    assert sorted({k[0] for k in es.slivers()}) == [(1, 1), (1, 200), (200, 1)]
    assert sorted({k[1] for k in es.slivers()}) == ["bilinear", "nearest"]
    for name in es.field_scenes():
        if name.startswith("sliver"):
            assert (es.expected(name).members > 0).any(), name


def test_trips_walks_a_second_trip_in_some_workgroups_only():
    s = es.trips()
    hw = s.obs.shape[1] * s.obs.shape[2]
    per_trip = es.HIST_MAX_STRIPS * es.BLOCK
    assert per_trip < hw < 2 * per_trip and hw % 64
    assert 0 < -(-(hw - per_trip) // es.BLOCK) < es.HIST_MAX_STRIPS


def test_many_planes_and_planted_inputs():
    s = es.many_planes()
    assert s.counts.shape == (4099, 2, 2, 3)
    hist, valid = es.expected_hist("many_planes")
    assert (valid > 0).sum() > 3000 and len({h.tobytes() for h in hist}) > 1000
    s = es.planted()
    M = s.n_members
    assert (s.counts > M).any() and (s.members < M).any() and (s.members > M).any() and np.isnan(s.obs).any() and s.mask.any()
    hist, valid = es.expected_hist("planted")
    clean = eo.histogram(np.minimum(s.counts, M), np.full_like(s.members, M), np.nan_to_num(s.obs, nan=1.0), None, M, s.thresholds)
    left_out = clean[1] - valid
    assert left_out.tolist() == [4 + 3, 3 + 1, 1 + 1 + 1]                    # planted counts / mask; members / NaN; each once
    for h, v in zip(hist, valid):
        assert (h.sum(axis=(1, 2)) == v).all()
