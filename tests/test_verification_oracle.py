"""The NumPy restatement of the verification contract (tests/verification_oracle.py) against scipy's box filter, against
answers known in closed form, and the bookkeeping of the C ABI -- all on the CPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import verification_oracle as vo
import verification_scenes as sc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("rg_contingency_f32", "rg_exceedance_sat_i32", "rg_fss_sums_i32", "rg_box_fraction_f32")


# ---- the window is scipy's uniform_filter -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.SCENES)
def test_window_counts_are_the_zero_padded_uniform_filter(name):
    ndimage = pytest.importorskip("scipy.ndimage")
    s, want = sc.scene(name), sc.expected(name)
    hit = vo.exceedance(s.forecast, s.thresholds, s.observed, s.mask)
    layers = [(0, 0), (hit.shape[0] - 1, hit.shape[1] - 1)]                 # first and last layer: scipy is the slow side
    for p, t in layers:
        for n in s.scales:
            box = ndimage.uniform_filter(hit[p, t].astype(np.float64), size=n, mode="constant", cval=0.0)
            assert np.array_equal(vo.window_counts(want.sat_f[p, t], n), np.rint(box * n * n).astype(np.int64)), (name, p, t, n)


def test_window_counts_by_brute_force_even_sizes_included():
    rng = np.random.default_rng(1)
    hit = rng.random((6, 9)) < 0.5
    table = hit.astype(np.int64).cumsum(0).cumsum(1)
    for n in (1, 2, 3, 4, 7, 255):
        want = np.zeros(hit.shape, dtype=np.int64)
        for y in range(6):
            for x in range(9):
                y0, x0 = y - n // 2, x - n // 2
                want[y, x] = hit[max(y0, 0):max(y0 + n, 0), max(x0, 0):max(x0 + n, 0)].sum()
        assert np.array_equal(vo.window_counts(table, n), want), n


# ---- known answers ------------------------------------------------------------------------------------------------------------
def _square(shape, y, x, side=6):
    a = np.zeros(shape, dtype=np.float32)
    a[y:y + side, x:x + side] = 40.0
    return a


def test_identical_fields_have_fss_exactly_one():
    s = sc.scene("rows")
    sums = vo.fss_sums(s.forecast, s.forecast, s.thresholds, s.scales, s.mask)
    assert (sums[..., 0] == 0).all() and (sums[..., 1] == sums[..., 2]).all() and (sums[..., 1] > 0).all()
    assert (vo.fss(sums) == 1.0).all()


def test_disjoint_fields_at_scale_one_have_fss_exactly_zero():
    f, o = _square((30, 40), 3, 4), _square((30, 40), 15, 20)
    sums = vo.fss_sums(f, o, (35.0,), (1,))
    assert sums[0, 0, 0].tolist() == [72, 36, 36] and vo.fss(sums)[0, 0, 0] == 0.0


def test_a_shifted_square_reaches_fss_one_where_the_window_covers_the_plane_and_never_falls_on_the_way():
    h, w = 30, 40
    f, o = _square((h, w), 10, 12), _square((h, w), 13, 19)                   # shifted by d = (3, 7)
    scales = (1, 2, 3, 5, 9, 15, 25, 41, 79, 255)
    score = vo.fss(vo.fss_sums(f, o, (35.0,), scales))[0, 0]
    assert score[0] == 0.0 and (np.diff(score) >= 0.0).all() and (score[:4] < 1.0).all()
    # from n = 2 * 40 - 1 the window of every pixel reaches 39 rows and columns to either side: it holds the whole plane
    assert score[-2] == 1.0 and score[-1] == 1.0


def test_contingency_and_scores_of_a_hand_made_case():
    f = np.float32([[40.0, 40.0, 10.0], [10.0, np.nan, 40.0]])
    o = np.float32([[40.0, 10.0, 40.0], [10.0, 40.0, np.inf]])
    c = vo.contingency(f, o, (35.0,))
    assert c.counts[0, 0].tolist() == [2, 1, 1] and c.valid.tolist() == [5]
    got = vo.scores(2, 1, 1, 1)
    chance = 3.0 * 3.0 / 5.0
    want = dict(pod=2 / 3, far=1 / 3, csi=2 / 4, bias=1.0, ets=(2 - chance) / (4 - chance), hss=2 * (2 - 1) / (3 * 2 + 3 * 2),
                base_rate=3 / 5)
    assert got.keys() == want.keys()
    for key, v in want.items():
        assert abs(float(got[key]) - v) < 1e-15, key
    masked = vo.contingency(f, o, (35.0,), np.uint8([[0, 7, 0], [0, 0, 0]]))
    assert masked.counts[0, 0].tolist() == [2, 0, 1] and masked.valid.tolist() == [4]
    empty = vo.scores(0, 0, 0, 0)
    assert all(np.isnan(v) for v in empty.values())


def test_thresholds_compare_inclusively_in_float32_and_minus_zero_is_zero():
    v = np.float32([[-0.0, 0.0, np.nextafter(np.float32(0), np.float32(-1)), -np.inf, np.inf, np.nan]])
    assert vo.exceedance(v, (0.0,))[0, 0, 0].tolist() == [True, True, False, False, True, False]
    assert vo.exceedance(v, (0.1,))[0, 0, 0].tolist() == [False, False, False, False, True, False]


def test_the_fraction_is_one_division():
    table = np.ones((4, 5), dtype=np.int64).cumsum(0).cumsum(1)
    got = vo.box_fraction(table, 3)
    assert got.dtype == np.float32 and got[1, 1] == 1.0 and got[0, 0] == np.float32(4.0 / 9.0)
    assert np.array_equal(vo.box_fraction(table, 1), np.ones((4, 5), dtype=np.float32))


# ---- ABI bookkeeping ----------------------------------------------------------------------------------------------------------
def test_abi_bookkeeping_and_exports():
    import radar_processor_amd as rg
    from radar_processor_amd import _native, build, verification
    header = open(os.path.join(REPO, "include", "radargrid_hip.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t|const char\*)\s+(rg_\w+)\s*\(", header, flags=re.M))
    assert "#define RG_VERSION 104" in header and _native.ABI_VERSION == 104
    assert "Nowcast verification" in header and "parity with pysteps unpinned" in header
    for define, value in (("RG_MAX_VERIFY_THRESHOLDS", 8), ("RG_MAX_VERIFY_SCALES", 16), ("RG_MAX_VERIFY_SCALE", 255)):
        assert f"#define {define} {value}" in header and getattr(_native, define) == value
    assert (verification.MAX_THRESHOLDS, verification.MAX_SCALES, verification.MAX_SCALE) == (vo.MAX_THRESHOLDS, vo.MAX_SCALES,
                                                                                            vo.MAX_SCALE) == (8, 16, 255)
    assert ("rg_verify.hip", []) in build.SOURCES
    lib = rg.load_library(require_device=False)
    for name in FUNCTIONS:
        assert name in declared and getattr(lib, name).argtypes == _native.SIGNATURES[name][1]
        args = re.search(r"^int %s\((.*?)\);" % name, header, flags=re.S | re.M).group(1).split(",")
        want = []
        for a in args:
            a = " ".join(a.split())
            want.append(ctypes.POINTER(ctypes.c_float) if a.startswith("const float* thresholds_host") else
                        ctypes.POINTER(ctypes.c_int32) if a.startswith("const int32_t* scales_host") else
                        ctypes.c_void_p if ("*" in a or a.startswith("rg_stream_t")) else ctypes.c_int32)
        assert want == _native.SIGNATURES[name][1], name
    for name in ("contingency_device", "categorical_scores", "exceedance_sat_device", "neighbourhood_fraction_device", "fss_device",
                 "verify_nowcast", "NowcastVerifier", "ContingencyTable", "FSSSums"):
        assert name in rg.__all__ and getattr(rg, name) is getattr(verification, name)
