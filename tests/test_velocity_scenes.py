"""The velocity scenes against the NumPy restatement, on the CPU: each scene reaches what it was built to reach, and the four
wind scenes named in ``velocity_scenes.RECOVERING`` come back with the true fold at EVERY valid gate.  The GPU tests assert
truth-recovery only on those four."""
import numpy as np
import pytest

import velocity_oracle as vo
import velocity_scenes as vs


@pytest.mark.parametrize("name", vs.RECOVERING)
def test_the_restatement_recovers_the_true_fold_at_every_valid_gate(name):
    s, ref = vs.scenes()[name], vs.reference(name)
    ok = vo.valid(s.vel)
    assert ok.sum() >= 0.85 * ok.size and np.abs(s.truth_folds[ok]).max() == 1            # the scene does fold, both ways
    assert np.array_equal(ref.folds[ok], s.truth_folds[ok])
    vn = float(s.nyquist)
    want = (s.vel.astype(np.float64) + s.truth_folds * (2.0 * vn)).astype(np.float32)
    assert np.array_equal(vo.bits(ref.velocity[ok]), vo.bits(want[ok])) and np.isnan(ref.velocity[~ok]).all()
    assert (ref.folds[~ok] == 0).all() and (ref.regions[~ok] == 0).all() and (ref.regions[ok] > 0).all()
    # dealiased, neighbouring valid gates differ by far less than the Nyquist velocity
    out = ref.velocity.astype(np.float64)
    step = np.abs(np.diff(out, axis=1))
    assert np.nanmax(step) < 0.5 * vn


@pytest.mark.parametrize("name", ["holes_25", "three_rays"])
def test_scenes_that_do_not_recover_are_kept_for_equality_only(name):
    """25 % holes leave isolated sets, three rays leave the centring little to go by: the restatement does NOT return the
    truth there, which is why no test asserts it."""
    full = vs.wind(36, 65, 8.0, 3, 19.0, holes=0.25, seed=1) if name == "holes_25" else vs.wind(3, 64, 10.0, 3, 22.0)
    ref = vs.reference(name)
    ok = vo.valid(full.vel)
    assert not np.array_equal(ref.folds[ok], full.truth_folds[ok])


def test_every_scene_reaches_what_it_was_built_for():
    sc = vs.scenes()
    ref = {name: vs.reference(name) for name in sc}
    assert ref["wind_1x1"].n_regions == 1 and len(ref["wind_1x1"].edges) == 0
    assert ref["wind_1x70"].n_regions >= 1 and ref["wind_70x1"].n_regions >= 2 and len(ref["wind_70x1"].edges) >= 2
    # h = 2: the wrap adds nothing; h = 3: it adds the seam's 64 pairs
    a, b = ref["rows_2x64_nowrap"], ref["rows_2x64_wrap"]
    assert np.array_equal(a.edges, b.edges) and np.array_equal(a.regions, b.regions) and a.edges[:, 2].sum() == 64
    a, b = ref["rows_3x64_nowrap"], ref["rows_3x64_wrap"]
    assert b.edges[:, 2].sum() == a.edges[:, 2].sum() + 64
    # two sweeps: no edge joins regions of different sweeps, and the sweeps' intervals differ
    two = ref["two_sweeps"]
    first = int(vo.regions(sc["two_sweeps"].vel, sc["two_sweeps"].nyquist, 3, sc["two_sweeps"].mask).cell_ptr[3])
    assert 0 < first < two.n_regions and ((two.edges[:, 0] <= first) == (two.edges[:, 1] <= first)).all()
    assert (two.regions[sc["two_sweeps"].mask != 0] == 0).all()
    # band limits: every band is hit, invalid gates carry no region
    s = sc["band_limits"]
    band = vo.bands(s.vel, s.nyquist, s.n_bands, s.mask)[0]
    assert set(np.unique(band)) == {-1, 0, 1, 2}
    bad = ~vo.valid(s.vel, s.mask)
    assert bad.sum() >= 10 and (ref["band_limits"].regions[bad] == 0).all() and np.isnan(ref["band_limits"].velocity[bad]).all()
    row = s.vel[0]
    e = np.float32(-10.0 + 20.0 / 3.0)
    at = int(np.nonzero(row == e)[0][0])
    assert row[at - 1] < e < row[at + 1] and band[0, at - 1] == 0 and band[0, at + 1] == 1
    assert band[0, int(np.nonzero(row == np.float32(10.0))[0][0])] == 2 and band[0, int(np.nonzero(row == np.float32(25.0))[0][0])] == 2
    assert band[0, int(np.nonzero(row == np.float32(-31.0))[0][0])] == 0
    # bands: 2 and 8 give other regions than 3
    assert ref["bands_8"].n_regions > ref["bands_2"].n_regions


def test_the_run_scenes_and_the_checkerboard():
    values, region = vs.two_regions("ray")
    e = vo.edges(values, region, True)
    assert e.shape == (1, 4) and e[0, 2] == 400 and abs(int(e[0, 3])) > 2 ** 32
    assert vo.edges(values, region, False)[0, 2] == 200
    values, region = vs.two_regions("gate", R=6)
    e = vo.edges(values, region, True)
    assert e.shape == (1, 4) and e[0, 2] == 6 and abs(int(e[0, 3])) > 2 ** 32
    s = vs.checkerboard()
    ref = vo.dealias(s.vel, s.nyquist, s.n_bands, None, s.wrap)
    R, G = s.vel.shape
    assert ref.n_regions == R * G and len(ref.edges) == R * (G - 1) + R * G and (ref.edges[:, 2] == 1).all()


def test_every_recorded_edge_count_respects_the_planar_bound():
    for name in vs.scenes():
        ref = vs.reference(name)
        if ref.n_regions >= 3:
            assert len(ref.edges) <= 3 * ref.n_regions - 6, name
    s = vs.checkerboard()
    ref = vo.dealias(s.vel, s.nyquist, s.n_bands, None, s.wrap)
    assert len(ref.edges) <= 3 * ref.n_regions - 6
