"""The scenes of the convection tests (tests/convection_scenes.py) under the NumPy restatement: the prefix oracle equals the
direct definition on every scene, the known answers hold, the main scenes populate every class and both centre criteria, and
no decision in them is fragile.  No GPU."""
import numpy as np
import pytest

import convection_oracle as co
import convection_scenes as sc
from radar_processor_amd.convection import disk_footprint


@pytest.mark.parametrize("name", [n for n in sc.SCENES if n != "big_sums"])
def test_the_prefix_oracle_equals_the_direct_definition(name):
    s, want = sc.scene(name), sc.expected(name)
    S, N, bkg = co.background(s.dbz, s.hw, s.mask, s.min_dbz, direct=True)
    assert np.array_equal(S, want.S) and np.array_equal(N, want.N)
    assert np.array_equal(bkg.view(np.uint32), want.bkg.view(np.uint32))
    classes, _, centres = co.classify(s.dbz, s.hw, s.footprints, s.edges, s.mask, s.min_dbz, s.intense, s.peak, direct=True)
    assert np.array_equal(centres, want.centres) and np.array_equal(classes, want.classes)
    assert np.array_equal(want.N > 0, ~np.isnan(want.bkg)) and (want.classes[~want.echo] == 0).all()
    assert (want.classes[want.centres > 0] == 2).all() and (want.centres[~want.echo] == 0).all()


def test_big_sums_pass_float64s_exact_integers_and_equal_the_closed_form():
    """The direct definition over 51 101 offsets of 67 600 pixels takes seconds, and the plane is uniform: the sum is q times
    the footprint's area inside the plane, which ``footprint_area`` counts row span by row span."""
    s, want = sc.scene("big_sums"), sc.expected("big_sums")
    q = 65536 * 10 ** 8                                                    # 85 dBZ clamps to 80
    assert (want.q == q).all() and want.echo.all()
    area = co.footprint_area(s.dbz.shape[1:], s.hw)
    assert np.array_equal(want.N[0], area) and np.array_equal(want.S[0], area * q)
    assert area.max() == area[130, 130] == 51101 and int(want.S.max()) > 3.3e17 > 2 ** 53 and int(want.S.max()) < 2 ** 59
    assert int(want.S.max()) % 2 == 0 and float(int(want.S.max()) + 1) == float(int(want.S.max()))     # float64 cannot count here
    assert (want.bkg == np.float32(80.0)).all() and (want.centres == 1).all() and (want.classes == 2).all()
    rows = np.array([0, 1, 129, 259])                                      # the direct definition on four rows of the plane
    for y in rows:
        lo, hi = max(y - 127, 0), min(y + 127, 259) + 1
        window = co.footprint_sum_direct(want.echo[:, lo:hi, :40], s.hw)   # 40 columns: the west rim and the interior
        assert np.array_equal(window[0, y - lo, :13], co.footprint_area((260, 40), s.hw)[y, :13]), y


def test_the_shapes_the_issue_names():
    shapes = {n: sc.scene(n).dbz.shape for n in sc.SCENES}
    assert shapes["main_35"] == shapes["main_39"] == (1, 72, 100) and shapes["stack"][0] == 3
    assert shapes["seam_257"] == (1, 70, 257) and shapes["seam_64"] == (1, 33, 64) and shapes["tall_disk"] == (1, 40, 150)
    assert shapes["big_sums"] == (1, 260, 260) and shapes["one_pixel"] == (1, 1, 1)
    assert shapes["one_row"] == (1, 1, 300) and shapes["one_column"] == (1, 300, 1)
    main = sc.scene("main_35")
    assert len(main.hw) - 1 == 22 and max(main.hw) == 27 and main.hw == disk_footprint(11000.0, sc.DY, sc.DX)
    assert main.footprints == tuple(disk_footprint(r, sc.DY, sc.DX) for r in sc.RADII)
    assert len(sc.scene("tall_disk").hw) - 1 == 127 and max(sc.scene("big_sums").hw) == 127
    stack = sc.expected("stack")
    assert not stack.echo[1].any() and stack.echo[0].any() and stack.echo[2].any() and not stack.classes[1].any()
    assert np.isnan(stack.bkg[1]).all()
    hw = sc.scene("non_monotone").hw
    assert any(a < b for a, b in zip(hw, hw[1:])) and any(a > b for a, b in zip(hw, hw[1:]))
    assert len(set(sc.scene("box").hw)) == 1
    assert all(np.nanmin(sc.scene(n).dbz) >= 0.0 for n in sc.SCENES)


@pytest.mark.parametrize("name", sc.MAIN)
def test_main_scenes_populate_every_class_and_both_criteria(name):
    s, want = sc.scene(name), sc.expected(name)
    assert np.isnan(s.dbz).mean() > 0.03 and 0.01 < (s.mask != 0).mean() < 0.03 and np.isnan(s.dbz[0, 20:45, :6]).all()
    assert (np.bincount(want.centres.ravel(), minlength=6)[1:] > 0).all(), np.bincount(want.centres.ravel()).tolist()
    _, by_intensity, by_peak = co.centres(s.dbz, want.bkg, s.edges, s.mask, s.min_dbz, s.intense, s.peak, return_criteria=True)
    assert (by_intensity & ~by_peak).any() and (by_peak & ~by_intensity).any()
    none, stratiform, convective = np.bincount(want.classes.ravel(), minlength=3)
    assert none > 400 and stratiform > 4000 and convective > 1000, (none, stratiform, convective)


@pytest.mark.parametrize("name", sc.MAIN)
def test_no_decision_in_a_main_scene_is_fragile(name):
    """Zero fragile decisions, no excluded share: the device's q may differ by a unit at a tie (at most 6.6e-5 dB in the mean)
    and its log10 by a float32 step (3.8e-6 dB), and 1e-3 dB leaves an order of magnitude over both -- so the device has to
    reproduce these scenes end to end, bit for bit."""
    intensity, peakedness, edge = sc.margins(name)
    assert intensity >= sc.FRAGILE_DB and peakedness >= sc.FRAGILE_DB and edge >= sc.FRAGILE_DB, (intensity, peakedness, edge)


# ---- known answers -------------------------------------------------------------------------------------------------------------
def _chain(planes, mask=None):
    s = sc.scene("main_35")
    return co.classify(planes, s.hw, s.footprints, s.edges, mask)


def test_uniform_20_dbz_is_all_stratiform_and_uniform_45_all_convective():
    classes, bkg, centres = _chain(sc.uniform(20.0))
    assert (classes == 1).all() and (centres == 0).all() and np.abs(bkg - 20.0).max() < 1e-5
    classes, bkg, centres = _chain(sc.uniform(45.0))
    assert (classes == 2).all() and (centres == 5).all() and np.abs(bkg - 45.0).max() < 1e-5


def test_a_spike_is_one_class_1_centre_whose_area_is_its_disk():
    planes, at = sc.spike()
    classes, bkg, centres = _chain(planes)
    assert centres.sum() == 1 and centres[0][at] == 1 and bkg[0][at] < 25.0
    disk = sc.footprint_mask(disk_footprint(1000.0, sc.DY, sc.DX), planes.shape[1:], at)
    assert disk.sum() == 5 + 5 + 5 + 1 + 1 and np.array_equal(classes[0] == 2, disk) and (classes[0][~disk] == 1).all()


def test_nothing_below_min_dbz_nan_or_masked_has_echo():
    planes = np.array([[[4.99, 5.0, np.nan, 50.0, 50.0]]], np.float32)
    mask = np.array([[[0, 0, 0, 9, 0]]], np.uint8)
    classes, bkg, centres = _chain(planes, mask)
    assert classes.tolist() == [[[0, 2, 0, 0, 2]]] and centres.tolist() == [[[0, 0, 0, 0, 5]]]
    assert not np.isnan(bkg).any()                                          # defined for every pixel with echo in reach
