"""CPU-side checks of the probabilistic nowcasts (no GPU needed): ``probability_scores`` against the scores formed pixel by
pixel, ``motion_perturbations``, the second header against ``_native.ENSEMBLE_SIGNATURES``, the exports, and the refusals of
the two entry points, all of which return before any HIP call."""
import ctypes
import os
import re

import numpy as np
import pytest

import radar_processor_amd as rg
from radar_processor_amd import _native, ensemble

import ensemble_oracle as eo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "radargrid_ensemble.h")
P = 1 << 12                                  # an aligned address that is never dereferenced
# Both sides are float64 sums over at most 10^4 pixels: the order of summation accounts for less than 1e-12 relative.
RTOL = 1e-10


def _pixels(seed, n, M, skill):
    """``(k, o)``: member counts and 0 / 1 observations of ``n`` pixels, the observation following the forecast when
    ``skill`` > 0."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, M + 1, size=n)
    p = skill * k / M + (1.0 - skill) * 0.3
    return k, (rng.random(n) < p).astype(np.int64)


def _table(k, o, M):
    return ensemble.ProbabilityTable(eo.table_from_pixels(k, o, M), np.array([len(k)]), M, np.array([35.0], np.float32))


# ---- scores --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,n,skill", [(1, 10, 0.6), (5, 1000, 0.8), (20, 10000, 0.5), (64, 9999, 0.0)])
def test_brier_score_and_its_decomposition_against_the_pixels(M, n, skill):
    k, o = _pixels(M * 7 + n, n, M, skill)
    s = rg.probability_scores(_table(k, o, M))
    direct = eo.brier_direct(k, o, M)
    assert s["brier"].shape == (1, 1) and direct > 0.01        # a Brier score of 0 is test_perfect_random_and_empty_tables'
    assert abs(s["brier"][0, 0] - direct) <= RTOL * direct
    assert abs(s["reliability"][0, 0] - s["resolution"][0, 0] + s["uncertainty"][0, 0] - s["brier"][0, 0]) <= RTOL * direct
    obar = o.mean()
    assert abs(s["base_rate"][0, 0] - obar) <= RTOL and abs(s["uncertainty"][0, 0] - obar * (1.0 - obar)) <= RTOL
    # the three terms from their definitions, pixel by pixel
    freq = np.array([o[k == j].mean() if (k == j).any() else np.nan for j in range(M + 1)])
    assert np.allclose(s["reliability_curve"][0, 0], freq, rtol=RTOL, atol=0.0, equal_nan=True)
    assert abs(s["reliability"][0, 0] - np.mean((k / M - freq[k]) ** 2)) <= RTOL
    assert abs(s["resolution"][0, 0] - np.mean((freq[k] - obar) ** 2)) <= RTOL
    assert abs(s["bss"][0, 0] - (1.0 - direct / (obar * (1.0 - obar)))) <= 1e-9
    assert np.array_equal(s["sharpness"][0, 0], np.bincount(k, minlength=M + 1)) and s["sharpness"].dtype == np.int64
    assert np.array_equal(s["forecast_probability"], np.arange(M + 1) / M)


@pytest.mark.parametrize("M,n,skill", [(5, 1000, 0.8), (20, 10000, 0.5)])
def test_roc_points_and_area(M, n, skill):
    k, o = _pixels(M + n, n, M, skill)
    s = rg.probability_scores(_table(k, o, M))
    pod, pofd = s["pod"][0, 0], s["pofd"][0, 0]
    assert pod.shape == (M + 2,)
    assert (pod[0], pofd[0]) == (1.0, 1.0) and (pod[-1], pofd[-1]) == (0.0, 0.0)
    for j in range(M + 2):
        warn = k >= j
        assert abs(pod[j] - (warn & (o == 1)).sum() / (o == 1).sum()) <= RTOL
        assert abs(pofd[j] - (warn & (o == 0)).sum() / (o == 0).sum()) <= RTOL
    assert (np.diff(pod) <= 0).all() and (np.diff(pofd) <= 0).all()
    assert abs(s["roc_area"][0, 0] - float(sum(0.5 * (pod[j] + pod[j + 1]) * (pofd[j] - pofd[j + 1]) for j in range(M + 1)))) <= RTOL
    assert s["roc_area"][0, 0] > 0.5                                          # these forecasts have skill


def test_perfect_random_and_empty_tables():
    M = 4
    k = np.array([0, 0, 4, 4, 0, 4])
    perfect = rg.probability_scores(_table(k, k // 4, M))
    assert perfect["brier"][0, 0] == 0.0 and perfect["bss"][0, 0] == 1.0 and perfect["roc_area"][0, 0] == 1.0
    never = rg.probability_scores(_table(k, np.zeros(6, np.int64), M))            # the event never happens
    assert never["uncertainty"][0, 0] == 0.0 and np.isnan(never["bss"][0, 0]) and np.isnan(never["pod"]).all()
    assert np.isnan(never["roc_area"][0, 0]) and not np.isnan(never["pofd"]).any()
    empty = rg.probability_scores(ensemble.ProbabilityTable(np.zeros((2, 3, M + 1, 2), np.int64), np.zeros(2, np.int64), M,
                                                            np.zeros(3, np.float32)))
    for key in ("brier", "reliability", "resolution", "uncertainty", "bss", "base_rate", "roc_area"):
        assert empty[key].shape == (2, 3) and np.isnan(empty[key]).all(), key
    assert np.isnan(empty["reliability_curve"]).all() and not empty["sharpness"].any()
    with pytest.raises(ValueError, match="ProbabilityTable"):
        rg.probability_scores(np.zeros((1, 1, 5, 2)))


def test_tables_add_and_refuse_what_does_not_add():
    a, b = _table(*_pixels(1, 500, 6, 0.5), 6), _table(*_pixels(2, 700, 6, 0.5), 6)
    total = a + b
    assert np.array_equal(total.hist, a.hist + b.hist) and total.valid.tolist() == [1200] and total.n_members == 6
    with pytest.raises(ValueError, match="do not add"):
        a + _table(*_pixels(3, 10, 5, 0.5), 5)
    with pytest.raises(ValueError, match="thresholds"):
        a + b._replace(thresholds=np.array([18.0], np.float32))


# ---- perturbations -------------------------------------------------------------------------------------------------------------
def test_motion_perturbations_shape_control_seed_and_closed_form():
    leads, par, perp = (0.0, 1.0, 2.0, 6.0), (1.2, 0.4, 0.3), (0.5, 0.7, 0.1)
    kw = dict(direction=(3.0, -4.0), par=par, perp=perp)
    s = rg.motion_perturbations(9, leads, seed=17, **kw)
    assert s.shape == (4, 9, 2) and s.dtype == np.float64 and np.isfinite(s).all()
    assert not s[:, 0].any() and not s[0].any() and s[1:, 1:].all()           # the control member, and lead 0
    assert np.array_equal(s, rg.motion_perturbations(9, leads, seed=17, **kw))
    assert not np.array_equal(s, rg.motion_perturbations(9, leads, seed=18, **kw))
    free = rg.motion_perturbations(9, leads, seed=17, control=False, **kw)
    assert free[1:, 0].all() and np.array_equal(free[:, 1:], s[:, 1:])
    # the closed form for member 3: the same two normal numbers at every lead
    z = np.random.default_rng(17).standard_normal((9, 2))[3]
    e_par, e_perp = np.array([0.6, -0.8]), np.array([-0.8, -0.6])
    for l, t in enumerate(leads):
        grown = [a * t ** (b + 1.0) / (b + 1.0) + c * t for a, b, c in (par, perp)]
        assert np.allclose(s[l, 3], z[0] * grown[0] * e_par + z[1] * grown[1] * e_perp, rtol=1e-13, atol=1e-15)
    back = rg.motion_perturbations(9, (-2.0,), seed=17, **kw)
    assert np.array_equal(back[0], -s[2])                                     # odd in the lead
    east = rg.motion_perturbations(2, (1.0,), direction=(0.0, 0.0), par=(1.0, 0.0, 0.0), perp=(0.0, 0.0, 0.0), seed=1)
    assert east[0, 1, 0] == 0.0 and east[0, 1, 1] != 0.0                      # a zero direction counts as eastward


@pytest.mark.parametrize("kw,match", [
    (dict(n_members=0), "n_members"), (dict(n_members=65), "n_members"), (dict(leads=(float("nan"),)), "leads"),
    (dict(par=(1.0, 2.0)), "par"), (dict(perp=(1.0, -1.0, 0.0)), "perp"), (dict(par=(float("inf"), 0.0, 0.0)), "par"),
    (dict(direction=(1.0,)), "direction"), (dict(direction=(float("nan"), 0.0)), "direction")])
def test_motion_perturbations_refusals(kw, match):
    args = dict(n_members=4, leads=(1.0,), direction=(1.0, 0.0), par=(1.0, 0.5, 0.0), perp=(1.0, 0.5, 0.0), seed=0)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        rg.motion_perturbations(args.pop("n_members"), args.pop("leads"), **args)
    with pytest.raises(TypeError):
        rg.motion_perturbations(4, (1.0,), direction=(1.0, 0.0), seed=0)      # par and perp have no default


# ---- the second header -----------------------------------------------------------------------------------------------------------
def _declared():
    """name -> [(C type, argument name)] of every function the header declares."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"^int\s+(rg_\w+)\s*\(([^;]*)\);", text, flags=re.M):
        out[name] = [tuple(a.strip().rsplit(" ", 1)) for a in args.replace("\n", " ").split(",")]
    return out


def _ctype(ctype, name):
    if name.endswith("_host"):
        return {"const float*": ctypes.POINTER(ctypes.c_float), "const double*": ctypes.POINTER(ctypes.c_double)}[ctype]
    if ctype.endswith("*") or ctype == "rg_stream_t":
        return ctypes.c_void_p
    return {"int32_t": ctypes.c_int32, "rg_motion_lattice": _native.MotionLattice}[ctype]


def test_header_and_table_mirror_each_other_one_to_one():
    declared = _declared()
    assert set(declared) == set(_native.ENSEMBLE_SIGNATURES) == {"rg_ensemble_exceedance_f32", "rg_ensemble_histogram_u8"}
    assert not set(declared) & set(_native.SIGNATURES)
    lib = rg.load_library(require_device=False)
    raw = ctypes.CDLL(_native.LIB_PATH)
    for name, args in declared.items():
        restype, argtypes = _native.ENSEMBLE_SIGNATURES[name]
        assert restype is ctypes.c_int32 and argtypes == [_ctype(*a) for a in args], name
        assert args[-1] == ("rg_stream_t", "stream"), f"{name}: the stream comes last"
        assert hasattr(raw, name), f"{name} declared in the header but not exported"
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    header = open(HEADER).read()
    assert '#include "radargrid_hip.h"' in header and f"#define RG_MAX_MEMBERS {_native.RG_MAX_MEMBERS}" in header
    assert lib.rg_version() == _native.ABI_VERSION == 104


def test_a_change_of_the_header_rebuilds_the_library():
    from radar_processor_amd import build
    assert ("rg_ensemble.hip", []) in build.SOURCES
    assert HEADER in build.sources_and_headers() and os.path.join(REPO, "include", "radargrid_hip.h") in build.sources_and_headers()


def test_exports():
    names = ["motion_perturbations", "ensemble_exceedance_device", "probabilistic_nowcast_device", "probabilistic_nowcast",
             "ensemble_histogram_device", "probability_scores", "EnsembleProducts", "ProbabilityTable"]
    for name in names:
        assert name in rg.__all__ and getattr(rg, name) is getattr(ensemble, name), name
    assert rg.EnsembleProducts._fields == ("prob", "counts", "members", "mean", "thresholds", "leads", "n_members")
    assert rg.ProbabilityTable._fields == ("hist", "valid", "n_members", "thresholds")


# ---- refusals of the C ABI: each returns before any HIP call ---------------------------------------------------------------------
def _lattice(**kw):
    f = dict(origin_y=0.0, origin_x=0.0, step_y=1.0, step_x=1.0, ny=4, nx=5)
    f.update(kw)
    return _native.MotionLattice(**f)


def exceedance_args(**kw):
    """A valid call of rg_ensemble_exceedance_f32 on addresses that are never dereferenced, with ``kw`` replacing arguments."""
    a = dict(src=P, h=4, w=5, motion=2 * P, lattice=_lattice(), leads=[1.0, 2.0], n_leads=None, substeps=1, method=0, shifts=3 * P,
             n_members=3, thresholds=[18.0, 35.0], n_thr=None, min_members=1, prob=16 * P, counts=32 * P, members=48 * P, mean=64 * P)
    a.update(kw)
    n_leads = len(a["leads"]) if a["n_leads"] is None else a["n_leads"]
    n_thr = len(a["thresholds"]) if a["n_thr"] is None else a["n_thr"]
    leads = (ctypes.c_double * max(len(a["leads"]), 1))(*a["leads"]) if a["leads"] is not None else None
    thr = (ctypes.c_float * max(len(a["thresholds"]), 1))(*a["thresholds"]) if a["thresholds"] is not None else None
    return (a["src"], a["h"], a["w"], a["motion"], a["lattice"], leads, n_leads, a["substeps"], a["method"], a["shifts"],
            a["n_members"], thr, n_thr, a["min_members"], a["prob"], a["counts"], a["members"], a["mean"], None)


NAN, INF = float("nan"), float("inf")
EXCEEDANCE_REFUSALS = [
    (dict(src=None), "null pointer"), (dict(motion=None), "null pointer"), (dict(shifts=None), "null pointer"),
    (dict(thresholds=None, n_thr=1), "null pointer"), (dict(leads=None, n_leads=1), "null pointer"),
    (dict(prob=None, counts=None, members=None, mean=None), "every output is NULL"),
    (dict(h=-1), "negative size -1 x 5"), (dict(w=-2), "negative size 4 x -2"),
    (dict(h=65536, w=32768), "h * w must stay below 2^31, got 65536 x 32768"),
    (dict(n_leads=-1), "n_leads must lie in 0 .. 16, got -1"), (dict(leads=[1.0] * 17), "n_leads must lie in 0 .. 16, got 17"),
    (dict(leads=[1.0, NAN]), "lead 1 is not finite"), (dict(leads=[INF]), "lead 0 is not finite"),
    (dict(lattice=_lattice(origin_x=NAN)), "a member of rg_motion_lattice is not finite"),
    (dict(lattice=_lattice(step_y=INF)), "a member of rg_motion_lattice is not finite"),
    (dict(lattice=_lattice(step_x=0.0)), "step_y and step_x must be positive"),
    (dict(lattice=_lattice(ny=0)), "ny and nx must be at least 1"),
    (dict(substeps=0), "substeps must lie in 1 .. 16, got 0"), (dict(substeps=17), "substeps must lie in 1 .. 16, got 17"),
    (dict(method=2), "unknown method 2"), (dict(method=-1), "unknown method -1"),
    (dict(n_members=0), "n_members must lie in 1 .. 64, got 0"), (dict(n_members=65), "n_members must lie in 1 .. 64, got 65"),
    (dict(thresholds=[], n_thr=0), "n_thr must lie in 1 .. 8, got 0"), (dict(thresholds=[1.0] * 9), "n_thr must lie in 1 .. 8, got 9"),
    (dict(thresholds=[1.0, INF]), "threshold 1 is not finite"), (dict(thresholds=[NAN]), "threshold 0 is not finite"),
    (dict(min_members=0), "min_members must lie in 1 .. n_members = 3, got 0"),
    (dict(min_members=4), "min_members must lie in 1 .. n_members = 3, got 4"),
    (dict(prob=P + 4), "prob overlaps src"), (dict(counts=2 * P + 159), "counts overlaps motion"),
    (dict(members=3 * P + 95), "members overlaps shifts"), (dict(mean=P), "mean overlaps src"),
    (dict(counts=16 * P + 319), "prob overlaps counts"), (dict(mean=16 * P), "prob overlaps mean"),
    (dict(members=32 * P + 79), "counts overlaps members"), (dict(mean=48 * P + 36), "members overlaps mean"),
]


@pytest.mark.parametrize("kw,message", EXCEEDANCE_REFUSALS)
def test_exceedance_refusals_name_the_function_and_the_reason(kw, message):
    lib = rg.load_library(require_device=False)
    assert lib.rg_ensemble_exceedance_f32(*exceedance_args(**kw)) == _native.RG_EINVAL
    assert lib.rg_last_error().decode() == "rg_ensemble_exceedance_f32: " + message


@pytest.mark.parametrize("kw", [dict(h=0), dict(w=0), dict(leads=[], n_leads=0), dict(leads=None, n_leads=0, shifts=None)])
def test_exceedance_of_nothing_is_ok_without_a_launch(kw):
    lib = rg.load_library(require_device=False)
    assert lib.rg_ensemble_exceedance_f32(*exceedance_args(**kw)) == _native.RG_OK


def test_exceedance_outputs_may_touch_without_overlapping():
    """2 leads x 2 thresholds x 20 pixels: prob is 320 bytes, counts 80, members 40.  With an empty plane every size is 0 and
    four equal addresses do not overlap; with the 4 x 5 plane counts one byte inside prob's end is refused (the list above),
    and counts AT prob's end is not what refuses the call below: the members inside counts are."""
    lib = rg.load_library(require_device=False)
    assert lib.rg_ensemble_exceedance_f32(*exceedance_args(h=0, prob=16 * P, counts=16 * P, members=16 * P, mean=16 * P)) == _native.RG_OK
    assert lib.rg_ensemble_exceedance_f32(*exceedance_args(counts=16 * P + 320, members=16 * P + 399)) == _native.RG_EINVAL
    assert lib.rg_last_error().decode() == "rg_ensemble_exceedance_f32: counts overlaps members"


def histogram_args(**kw):
    a = dict(counts=P, members=2 * P, obs=3 * P, mask=4 * P, n_planes=2, h=4, w=5, n_members=3, thresholds=[18.0, 35.0], n_thr=None,
             hist=16 * P, valid=32 * P)
    a.update(kw)
    n_thr = len(a["thresholds"]) if a["n_thr"] is None else a["n_thr"]
    thr = (ctypes.c_float * max(len(a["thresholds"]), 1))(*a["thresholds"]) if a["thresholds"] is not None else None
    return (a["counts"], a["members"], a["obs"], a["mask"], a["n_planes"], a["h"], a["w"], a["n_members"], thr, n_thr, a["hist"],
            a["valid"], None)


HISTOGRAM_REFUSALS = [
    (dict(counts=None), "null pointer"), (dict(members=None), "null pointer"), (dict(obs=None), "null pointer"),
    (dict(hist=None), "null pointer"), (dict(valid=None), "null pointer"), (dict(thresholds=None, n_thr=1), "null pointer"),
    (dict(n_planes=0), "n_planes must lie in 1 .. 65535, got 0"), (dict(n_planes=65536), "n_planes must lie in 1 .. 65535, got 65536"),
    (dict(h=-1), "negative size -1 x 5"), (dict(h=65536, w=32768), "h * w must stay below 2^31, got 65536 x 32768"),
    (dict(n_members=0), "n_members must lie in 1 .. 64, got 0"), (dict(n_members=65), "n_members must lie in 1 .. 64, got 65"),
    (dict(thresholds=[1.0] * 9), "n_thr must lie in 1 .. 8, got 9"), (dict(thresholds=[NAN]), "threshold 0 is not finite"),
    (dict(valid=16 * P + 255), "hist overlaps valid"), (dict(hist=P + 79), "an output overlaps counts"),
    (dict(valid=2 * P + 39), "an output overlaps members"), (dict(hist=3 * P + 159), "an output overlaps obs"),
    (dict(valid=4 * P), "an output overlaps mask"),
]


@pytest.mark.parametrize("kw,message", HISTOGRAM_REFUSALS)
def test_histogram_refusals_name_the_function_and_the_reason(kw, message):
    lib = rg.load_library(require_device=False)
    assert lib.rg_ensemble_histogram_u8(*histogram_args(**kw)) == _native.RG_EINVAL
    assert lib.rg_last_error().decode() == "rg_ensemble_histogram_u8: " + message


# ---- refusals of the wrappers: ValueError before the library is loaded -------------------------------------------------------------
def test_wrapper_refusals():
    plane = np.zeros((6, 7), np.float32)
    motion = np.zeros((6, 7, 2), np.float32)
    shifts = np.zeros((2, 3, 2))
    ok = dict(plane=plane, motion=motion, leads=(1.0, 2.0), shifts=shifts, thresholds=(18.0,))

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return rg.ensemble_exceedance_device(a.pop("plane"), a.pop("motion"), a.pop("leads"), a.pop("shifts"), a.pop("thresholds"), **a)

    for kw, match in [(dict(plane=np.zeros((1, 6, 7), np.float32)), r"one float32 \[h, w\] plane"),
                      (dict(plane=plane.astype(np.float64)), "plane must be float32"),
                      (dict(shifts=shifts.astype(np.float32)), "shifts must be float64"),
                      (dict(shifts=np.zeros((3, 3, 2))), "for 2 leads"), (dict(shifts=np.zeros((2, 65, 2))), "1 .. 64 members"),
                      (dict(shifts=np.full((2, 3, 2), np.nan)), "NaN or inf"), (dict(thresholds=()), "thresholds"),
                      (dict(thresholds=(np.nan,)), "finite"), (dict(method="cubic"), "method"), (dict(substeps=0), "substeps"),
                      (dict(min_members=4), "min_members"), (dict(min_members=0), "min_members"), (dict(want=()), "want"),
                      (dict(want=("prob", "spread")), "want"), (dict(want=("prob", "prob")), "want"),
                      (dict(leads=(np.inf,), shifts=shifts[:1]), "leads"),
                      (dict(motion=np.full((6, 7, 2), np.nan, np.float32)), "NaN or inf")]:
        with pytest.raises(ValueError, match=match):
            call(**kw)
    with pytest.raises(ValueError, match="unknown keyword"):
        rg.probabilistic_nowcast_device(plane, plane, (1.0,), (18.0,), 4, par=(1, 0, 0), perp=(1, 0, 0), seed=0, fill_value=0.0)
    with pytest.raises(ValueError, match="n_members"):
        rg.probabilistic_nowcast_device(plane, plane, (1.0,), (18.0,), 0, par=(1, 0, 0), perp=(1, 0, 0), seed=0)
    with pytest.raises(ValueError, match="min_members"):
        rg.probabilistic_nowcast_device(plane, plane, (1.0,), (18.0,), 4, par=(1, 0, 0), perp=(1, 0, 0), seed=0, min_members=5)
    with pytest.raises(TypeError):
        rg.probabilistic_nowcast_device(plane, plane, (1.0,), (18.0,), 4, seed=0)
    products = ensemble.EnsembleProducts(None, None, None, None, np.array([18.0], np.float32), (1.0,), 3)
    with pytest.raises(ValueError, match="counts"):
        rg.ensemble_histogram_device(products, plane)
    with pytest.raises(ValueError, match="EnsembleProducts"):
        rg.ensemble_histogram_device((None,) * 7, plane)
    full = products._replace(counts=np.zeros((1, 1, 6, 7), np.uint8), members=np.zeros((1, 6, 7), np.uint8))
    with pytest.raises(ValueError, match="observed"):
        rg.ensemble_histogram_device(full, np.zeros((2, 6, 7), np.float32))
    with pytest.raises(ValueError, match="mask"):
        rg.ensemble_histogram_device(full, plane, mask=np.zeros((5, 7), np.uint8))
    with pytest.raises(ValueError, match="counts must be uint8"):
        rg.ensemble_histogram_device(full._replace(counts=np.zeros((1, 2, 6, 7), np.uint8)), plane)
