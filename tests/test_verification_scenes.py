"""The verification scenes (tests/verification_scenes.py) through the NumPy restatement (tests/verification_oracle.py), on the
CPU: that the scenes hold what they claim, so that no GPU test built on them is vacuous; that every entry point turns a bad
argument away before it touches the device; and that the Python functions name the argument they refuse."""
import ctypes

import numpy as np
import pytest

import verification_oracle as vo
import verification_scenes as sc


# ---- the scenes hold what they claim ------------------------------------------------------------------------------------------
def test_the_shapes_cross_every_trip_boundary():
    shapes = {name: sc.scene(name).forecast.shape for name in sc.SCENES}
    assert shapes["rim"] == (1, 5, 7) and shapes["rows"] == (3, 45, 150) and shapes["many"] == (2, 700, 600)
    assert shapes["line_h"] == (1, 1, 200) and shapes["line_v"] == (1, 200, 1) and shapes["big_sums"] == (1, 300, 300)
    w = shapes["rows"][2]
    assert 2 * sc.WAVE < w < 3 * sc.WAVE and w % 4                           # three trips: the row carry is crossed twice
    assert len(sc.scene("rows").thresholds) == vo.MAX_THRESHOLDS and sc.scene("rows").scales == (1, 2, 3, 8, 31, 64, 255)
    assert sc.scene("rim").scales == (1, 2, 3, 255) and sc.scene("many").scales == (1, 16, 129)
    for name in sc.SCENES:
        s = sc.scene(name)
        assert not s.forecast.flags.writeable and not s.observed.flags.writeable
        assert s.forecast.dtype == np.float32 and s.observed.shape == s.forecast.shape


def test_rim_windows_are_cut_by_the_border_and_the_last_covers_the_plane():
    s, want = sc.scene("rim"), sc.expected("rim")
    h, w = s.forecast.shape[1:]
    for n in s.scales[1:]:
        area = np.outer(sc.clipped_span(h, n), sc.clipped_span(w, n))
        assert (area[0] < n * n).all() and (area[:, 0] < n * n).all(), n                    # the rim cuts them
        assert (area[-1] < n * n).all() == (n > 2) and (area < n * n).all() == (n == 255), n      # an even window reaches back
    assert (sc.clipped_span(h, 255) == h).all() and (sc.clipped_span(w, 255) == w).all()
    everything = want.sat_f[0, 0, -1, -1]
    assert 0 < everything < h * w and (vo.window_counts(want.sat_f[0, 0], 255) == everything).all()


def test_rows_holds_ties_both_infinities_minus_zero_and_nans_at_different_pixels():
    s, want = sc.scene("rows"), sc.expected("rows")
    for field in (s.forecast, s.observed):
        for t in s.thresholds:
            assert (field == np.float32(t)).any(), t                          # a value exactly at every threshold
        assert np.isposinf(field).any() and np.isneginf(field).any()
        assert (np.signbit(field) & (field == 0.0)).any() and (~np.signbit(field) & (field == 0.0)).any()
        assert 0.03 < np.isnan(field).mean() < 0.07
    nan_f, nan_o = np.isnan(s.forecast), np.isnan(s.observed)
    assert (nan_f & ~nan_o).any() and (~nan_f & nan_o).any()
    assert 0.02 < (s.mask != 0).mean() < 0.04 and len(np.unique(s.mask)) > 20      # any non-zero byte excludes
    # pairwise: a forecast pixel whose observation is NaN, or that is masked, exceeds nothing
    alone = vo.sat(s.forecast, s.thresholds)
    assert (alone[:, :, -1, -1] > want.sat_f[:, :, -1, -1]).all()
    assert (want.counts > 0).all() and (want.valid < 45 * 150).all() and (want.valid > 0).all()
    # -0.0 exceeds 0.0, and -inf nothing
    assert want.sat_f[0, 0, -1, -1] > want.sat_f[0, 1, -1, -1] > 0


def test_none_and_all_are_what_their_names_say():
    s, want = sc.scene("none"), sc.expected("none")
    assert not want.counts.any() and not want.sums.any() and not want.sat_f.any() and want.valid.tolist() == [45 * 150]
    assert np.isnan(vo.fss(want.sums)).all()
    s, want = sc.scene("all"), sc.expected("all")
    assert (want.counts[..., 0] == 45 * 150).all() and not want.counts[..., 1:].any()
    for k, n in enumerate(s.scales):
        closed = sc.sum_of_squared_areas(45, 150, n)
        assert want.sums[0, :, k].tolist() == [[0, closed, closed]] * 2, n
    assert sc.sum_of_squared_areas(45, 150, 1) == 45 * 150 and sc.sum_of_squared_areas(45, 150, 255) < (45 * 150) ** 3


def test_big_sums_outgrows_31_bits_per_pixel_and_47_in_total():
    """The largest square a pixel can add is 255^4 = 4 228 250 625: above 2^31, so a signed 32-bit product wraps, and 1.6 % below
    2^32, which no window of at most 255 x 255 reaches.  The total outgrows 2^32 some 37 000 times."""
    s, want = sc.scene("big_sums"), sc.expected("big_sums")
    cf = vo.window_counts(want.sat_f[0, 0], 255)
    assert int(cf.max()) == 255 * 255 and 2 ** 31 < int(cf.max()) ** 2 < 2 ** 32 and not want.sat_o.any()
    closed = sc.sum_of_squared_areas(300, 300, 255)
    assert closed == 12598700 ** 2 > 2 ** 47
    assert want.sums[0, 0, 0].tolist() == [closed, closed, 0]
    exact = vo.fss_sums(s.forecast, s.observed, s.thresholds, s.scales, python_ints=True)
    assert [int(v) for v in exact[0, 0, 0]] == [closed, closed, 0]
    assert vo.fss(want.sums)[0, 0, 0] == 0.0


def test_many_has_tables_in_the_hundred_thousands_and_int64_did_not_wrap():
    s, want = sc.scene("many"), sc.expected("many")
    assert want.sat_f[:, 0, -1, -1].min() > 100000 and want.sat_f[:, -1, -1, -1].min() > 10000
    assert (want.sums[..., 0] > 0).all() and (want.counts > 0).all()
    exact = vo.fss_sums(s.forecast[:1], s.observed[:1], s.thresholds[:1], (129,), s.mask[:1], python_ints=True)
    assert [int(v) for v in exact[0, 0, 0]] == want.sums[0, 0, 2].tolist()
    score = vo.fss(want.sums)
    assert (np.diff(score, axis=-1) > 0).all() and (score > 0).all() and (score < 1).all()


def test_the_blob_sequence_moves_exactly_and_keeps_its_margin():
    frames = sc.blob_sequence()
    assert frames.shape == (sc.SEQ_FRAMES,) + sc.SEQ_SHAPE
    dy, dx = sc.SEQ_MOTION
    for k in range(sc.SEQ_FRAMES):
        ys, xs = np.nonzero(frames[k] > 5.0)
        assert ys.min() >= sc.SEQ_MARGIN and ys.max() <= sc.SEQ_SHAPE[0] - 1 - sc.SEQ_MARGIN
        assert xs.min() >= sc.SEQ_MARGIN and xs.max() <= sc.SEQ_SHAPE[1] - 1 - sc.SEQ_MARGIN
        if k:
            assert np.array_equal(np.roll(frames[k - 1], (dy, dx), axis=(0, 1)), frames[k])
    for t in sc.SEQ_THRESHOLDS[:-1]:
        assert (frames[0] >= t).any()
    assert not (frames >= sc.SEQ_THRESHOLDS[-1]).any()


# ---- every entry point turns a bad argument away before the device ------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import radar_processor_amd as rg
    return rg.load_library(require_device=False)


EINVAL = -1
P = 4096                                       # a pointer that is never followed: every call below fails its checks first


def _thr(*values):
    return (ctypes.c_float * max(len(values), 1))(*values)


def _scales(*values):
    return (ctypes.c_int32 * max(len(values), 1))(*values)


def test_contingency_rejects(lib):
    good = _thr(18.0, 35.0)
    call = lib.rg_contingency_f32
    assert call(0, P, 0, 1, 4, 4, good, 2, P, P + 4096, 0) == EINVAL and b"null" in lib.rg_last_error()
    assert call(P, P, 0, 1, 4, 4, good, 2, 0, P + 4096, 0) == EINVAL
    assert call(P, P, 0, 1, 4, 4, good, 2, P + 4096, 0, 0) == EINVAL
    assert call(P, P, 0, 1, 4, 4, None, 2, P + 4096, P + 8192, 0) == EINVAL
    for n_thr in (0, 9, -1):
        assert call(P, P, 0, 1, 4, 4, _thr(*range(9)), n_thr, P + 4096, P + 8192, 0) == EINVAL and b"n_thr" in lib.rg_last_error()
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert call(P, P, 0, 1, 4, 4, _thr(18.0, bad), 2, P + 4096, P + 8192, 0) == EINVAL and b"finite" in lib.rg_last_error()
    assert call(P, P, 0, 0, 4, 4, good, 2, P + 4096, P + 8192, 0) == EINVAL
    assert call(P, P, 0, 1, -1, 4, good, 2, P + 4096, P + 8192, 0) == EINVAL
    assert call(P, P, 0, 1, 46341, 46341, good, 2, 1 << 40, (1 << 40) + 4096, 0) == EINVAL and b"2^31" in lib.rg_last_error()


def test_exceedance_sat_rejects(lib):
    good = _thr(18.0)
    call = lib.rg_exceedance_sat_i32
    assert call(0, 0, 0, 1, 4, 4, good, 1, P, 0) == EINVAL and b"null" in lib.rg_last_error()
    assert call(P, 0, 0, 1, 4, 4, good, 1, 0, 0) == EINVAL
    assert call(P, 0, 0, 1, 4, 4, None, 1, P + 4096, 0) == EINVAL
    for n_thr in (0, 9):
        assert call(P, 0, 0, 1, 4, 4, _thr(*range(9)), n_thr, P + 4096, 0) == EINVAL and b"n_thr" in lib.rg_last_error()
    assert call(P, 0, 0, 1, 4, 4, _thr(float("nan")), 1, P + 4096, 0) == EINVAL and b"finite" in lib.rg_last_error()
    assert call(P, 0, 0, 1, 46341, 46341, good, 1, 1 << 40, 0) == EINVAL and b"2^31" in lib.rg_last_error()
    assert call(P, 0, 0, 1, 4, 4, good, 1, P + 32, 0) == EINVAL and b"overlaps" in lib.rg_last_error()


def test_fss_sums_rejects(lib):
    call = lib.rg_fss_sums_i32
    far = 1 << 40
    assert call(0, P, 1, 4, 4, _scales(1), 1, far, 0) == EINVAL and b"null" in lib.rg_last_error()
    assert call(P, P, 1, 4, 4, None, 1, far, 0) == EINVAL
    assert call(P, P, 1, 4, 4, _scales(1), 1, 0, 0) == EINVAL
    for n_scales in (0, 17):
        assert call(P, P, 1, 4, 4, _scales(*range(1, 18)), n_scales, far, 0) == EINVAL and b"n_scales" in lib.rg_last_error()
    for bad in (0, 256, -3):
        assert call(P, P, 1, 4, 4, _scales(1, bad), 2, far, 0) == EINVAL and b"scale" in lib.rg_last_error()
    # the overflow rule: min(n^2, h * w)^2 * h * w reaches 2^63 at 50000 x 50000 under scale 255, and the int32 tables end
    # at 2^31 pixels before that
    assert 65025 ** 2 * 50000 * 50000 >= 2 ** 63 > 65025 ** 2 * (2 ** 31 - 1)
    assert call(P, P, 1, 50000, 50000, _scales(255), 1, far, 0) == EINVAL
    assert call(P, P, 1, 46341, 46341, _scales(255), 1, far, 0) == EINVAL and b"2^31" in lib.rg_last_error()


def test_box_fraction_rejects(lib):
    call = lib.rg_box_fraction_f32
    far = 1 << 40
    assert call(0, 1, 4, 4, 3, far, 0) == EINVAL and b"null" in lib.rg_last_error()
    assert call(P, 1, 4, 4, 3, 0, 0) == EINVAL
    for bad in (0, 256):
        assert call(P, 1, 4, 4, bad, far, 0) == EINVAL and b"scale" in lib.rg_last_error()
    assert call(P, 0, 4, 4, 3, far, 0) == EINVAL
    assert call(P, 1, 46341, 46341, 3, far, 0) == EINVAL and b"2^31" in lib.rg_last_error()
    assert call(P, 1, 4, 4, 3, P + 16, 0) == EINVAL and b"overlaps" in lib.rg_last_error()


# ---- Python argument errors name the argument ---------------------------------------------------------------------------------
def test_python_argument_errors_name_the_argument():
    import radar_processor_amd as rg
    f = np.zeros((2, 4, 5), dtype=np.float32)
    with pytest.raises(ValueError, match="forecast"):
        rg.contingency_device(f.astype(np.float64), f, (18.0,))
    with pytest.raises(ValueError, match="observed"):
        rg.contingency_device(f, f[:1], (18.0,))
    with pytest.raises(ValueError, match="mask"):
        rg.contingency_device(f, f, (18.0,), mask=np.zeros((4, 5), dtype=np.uint8))
    for bad in ((), tuple(range(9)), (float("nan"),), (float("inf"),), (1e39,), ("x",)):
        with pytest.raises(ValueError, match="thresholds"):
            rg.contingency_device(f, f, bad)
    with pytest.raises(ValueError, match="partner"):
        rg.exceedance_sat_device(f, (18.0,), partner=f[0])
    for bad in (0, 256, 2.0, True):
        with pytest.raises(ValueError, match="scale"):
            rg.neighbourhood_fraction_device(f, (18.0,), bad)
    for bad in ((), tuple(range(1, 18)), (0,), (3, 256), (1.5,)):
        with pytest.raises(ValueError, match="scales"):
            rg.fss_device(f, f, (18.0,), bad)
    with pytest.raises(ValueError, match="observations"):
        rg.verify_nowcast(f, f[0], (18.0,), (1,))
    with pytest.raises(ValueError, match="ContingencyTable"):
        rg.categorical_scores((1, 2, 3, 4, 5))
    for bad in ((), (0,), (1, 1), (1.5,), tuple(range(1, 18))):
        with pytest.raises(ValueError, match="lead_frames"):
            rg.NowcastVerifier(bad, (18.0,), (1,))
    with pytest.raises(ValueError, match="motion"):
        rg.NowcastVerifier((1,), (18.0,), (1,), motion="manual")
    with pytest.raises(ValueError, match="block"):
        rg.NowcastVerifier((1,), (18.0,), (1,), motion=None, block=32)
    with pytest.raises(ValueError, match="fill_value"):
        rg.NowcastVerifier((1,), (18.0,), (1,), fill_value=0.0)
    with pytest.raises(ValueError, match="method"):
        rg.NowcastVerifier((1,), (18.0,), (1,), method="cubic")
    with pytest.raises(ValueError, match="substeps"):
        rg.NowcastVerifier((1,), (18.0,), (1,), substeps=17)
    verifier = rg.NowcastVerifier((1, 2), (18.0, 35.0), (1, 9), motion=None)
    assert verifier.lead_frames == (1, 2) and verifier.scales == (1, 9) and verifier.totals() is None
    with pytest.raises(ValueError, match="plane"):
        verifier.update(f)
    with pytest.raises(ValueError, match="kind"):
        verifier.totals("climatology")
    assert verifier.scores()["nowcast"] is None


def test_tables_and_sums_add_exactly_and_scores_never_raise():
    import radar_processor_amd as rg
    big = np.int64(2 ** 62)
    a = rg.ContingencyTable(*(np.full((1, 2), v, dtype=np.int64) for v in (3, 1, 2, 4)), np.array([10], dtype=np.int64))
    total = a + a
    assert isinstance(total, rg.ContingencyTable) and total.hits.tolist() == [[6, 6]] and total.valid.tolist() == [20]
    with pytest.raises(ValueError, match="do not add"):
        a + rg.ContingencyTable(*(np.zeros((2, 2), dtype=np.int64),) * 4, np.zeros(2, dtype=np.int64))
    with pytest.raises(TypeError):
        a + (1, 2, 3, 4, 5)
    got, want = rg.categorical_scores(a), vo.scores(3, 1, 2, 4)
    for key, v in want.items():
        assert got[key].shape == (1, 2) and (got[key] == v).all(), key
    zero = rg.categorical_scores(rg.ContingencyTable(*(np.zeros((1, 1), dtype=np.int64),) * 4, np.zeros(1, dtype=np.int64)))
    assert all(np.isnan(v).all() for v in zero.values())
    s = rg.FSSSums(np.array([[[[big // 2, big, big - 1], [0, 0, 0], [0, 5, 5]]]], dtype=np.int64), np.array([[30]], dtype=np.int64),
                   np.array([100], dtype=np.int64))
    assert (s + s).pixels.tolist() == [200] and (s + s).sums[0, 0, 2].tolist() == [0, 10, 10]
    score = s.fss()
    assert score.shape == (1, 1, 3) and np.isnan(score[0, 0, 1]) and score[0, 0, 2] == 1.0 and abs(score[0, 0, 0] - 0.75) < 1e-12
    assert abs(s.useful()[0, 0] - 0.65) < 1e-15 and abs((s + s).useful()[0, 0] - 0.65) < 1e-15
