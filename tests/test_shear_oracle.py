"""CPU-side checks of the shear products (no GPU needed): the fifth header against ``_native.SHEAR_SIGNATURES``, the build lists,
the exports, the refusals of the wrappers and of the entry points (all of which return before any HIP call), the vectorised
restatement against the naive one, and ``llsd_window`` against values worked out by hand."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import radar_processor_amd as rg
from radar_processor_amd import _native, shear

import shear_oracle as so
import shear_scenes as ss

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "radargrid_shear.h")
NAMES = {"rg_polar_median_f32", "rg_velocity_llsd_f32"}
MACROS = ("RG_SHEAR_MEDIAN_MAX_HALF", "RG_SHEAR_MAX_HALF_RAYS", "RG_SHEAR_MAX_HALF_GATES", "RG_SHEAR_MAX_WINDOW")
P = 1 << 20                                  # an aligned address that is never dereferenced
NAN, INF = float("nan"), float("inf")


# ---- the fifth header ------------------------------------------------------------------------------------------------------------
def _declared():
    """name -> (return type, [(C type, argument name)]) of every function the header declares."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"^(int|int64_t)\s+(rg_\w+)\s*\(([^;]*)\);", text, flags=re.M):
        out[name] = (ret, [tuple(a.strip().rsplit(" ", 1)) for a in args.replace("\n", " ").split(",")])
    return out


def _ctype(ctype, name):
    assert not name.endswith("_host")            # neither entry point reads an array on the host
    if ctype.endswith("*") or ctype == "rg_stream_t":
        return ctypes.c_void_p
    return {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}[ctype]


def test_header_and_table_mirror_each_other_one_to_one():
    declared = _declared()
    assert set(declared) == set(_native.SHEAR_SIGNATURES) == NAMES
    for table in (_native.SIGNATURES, _native.ENSEMBLE_SIGNATURES, _native.PHASE_SIGNATURES, _native.VELOCITY_SIGNATURES):
        assert not NAMES & set(table)
    lib = rg.load_library(require_device=False)
    raw = ctypes.CDLL(_native.LIB_PATH)
    for name, (ret, args) in declared.items():
        restype, argtypes = _native.SHEAR_SIGNATURES[name]
        assert restype is {"int": ctypes.c_int32, "int64_t": ctypes.c_int64}[ret], name
        assert argtypes == [_ctype(*a) for a in args], name
        assert args[-1] == ("rg_stream_t", "stream"), f"{name}: the stream comes last"
        assert hasattr(raw, name), f"{name} declared in the header but not exported"
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    header = open(HEADER).read()
    assert '#include "radargrid_hip.h"' in header and '#include "radargrid_velocity.h"' in header
    for macro in MACROS:
        assert re.search(r"#define %s %d\b" % (macro, getattr(_native, macro)), header), macro
    assert _native.RG_SHEAR_MAX_WINDOW == (2 * _native.RG_SHEAR_MAX_HALF_RAYS + 1) * (2 * _native.RG_SHEAR_MAX_HALF_GATES + 1)
    assert lib.rg_version() == _native.ABI_VERSION == 104


def test_the_new_unit_and_header_are_part_of_the_build_and_the_pinned_lists_are_unchanged():
    from radar_processor_amd import build
    assert ("rg_shear.hip", []) in build.SOURCES and build.SOURCES[-1] == ("rg_warp.hip", [])
    assert build.SOURCES.index(("rg_shear.hip", [])) == build.SOURCES.index(("rg_velocity.hip", [])) + 1
    assert build.PUBLIC_HEADERS == ["radargrid_hip.h", "radargrid_ensemble.h", "radargrid_phase.h"]
    assert build.POLAR_HEADERS == ["radargrid_velocity.h"]
    assert build.SHEAR_HEADERS == ["radargrid_shear.h"]
    files = build.sources_and_headers()
    assert HEADER in files and os.path.join(build.CSRC, "rg_shear.hip") in files
    assert files.index(HEADER) > files.index(os.path.join(build.INCLUDE, "radargrid_velocity.h"))
    assert set(_native.VELOCITY_SIGNATURES) == {"rg_velocity_split_f32", "rg_velocity_regions_i32", "rg_region_edges_workspace_bytes",
                                                "rg_region_edges_f32", "rg_velocity_apply_folds_f32"}
    assert set(_native.PHASE_SIGNATURES) == {"rg_phidp_unfold_f32", "rg_phidp_fit_f32", "rg_attenuation_phidp_f32"}


def test_exports():
    names = ["llsd_window", "median_filter_device", "velocity_shear_device", "azimuthal_shear_device", "velocity_shear",
             "ShearWindow", "VelocityShear"]
    for name in names:
        assert name in rg.__all__ and getattr(rg, name) is getattr(shear, name), name
    assert rg.ShearWindow._fields == ("half_rays", "az_scale", "max_half_rays", "half_gates", "range_scale")
    assert rg.VelocityShear._fields == ("azimuthal_shear", "radial_divergence", "velocity", "count")
    assert (shear.MEDIAN_MAX_HALF, shear.MAX_HALF_RAYS, shear.MAX_HALF_GATES, shear.MAX_WINDOW) == (2, 16, 16, 1089)


# ---- llsd_window -------------------------------------------------------------------------------------------------------------------
def test_llsd_window_against_hand_computed_values():
    r = np.array([0.0, -5.0, 1000.0, 20000.0, 35809.9, 35810.0, 60000.0, 200000.0])
    w = rg.llsd_window(r, 1.0, 250.0)
    assert isinstance(w, rg.ShearWindow) and w.half_rays.dtype == np.int32 and w.az_scale.dtype == np.float64
    dtheta = math.pi / 180.0
    # 2500 / (2 r dtheta) = 71619.7 / r: 71.6 -> clipped to 16; 3.58 -> 4; 2.000003 and 1.999997 -> 2; 1.19 -> 1; 0.36 -> clipped to 1
    assert w.half_rays.tolist() == [0, 0, 16, 4, 2, 2, 1, 1]
    assert w.az_scale[0] == 0.0 and w.az_scale[1] == 0.0
    assert w.az_scale[2] == 1.0 / (65536.0 * (1000.0 * dtheta)) and w.az_scale[7] == 1.0 / (65536.0 * (200000.0 * dtheta))
    assert w.max_half_rays == 16 and w.half_gates == 2 and w.range_scale == 1.0 / (65536.0 * 250.0)        # floor(1.5 + 0.5)
    # the half sits on the round-up side: 2500 / (2 r dtheta) = 2.5 exactly at r = 500 / dtheta
    assert rg.llsd_window(np.array([500.0 / dtheta * (1 - 1e-12), 500.0 / dtheta * (1 + 1e-12)]), 1.0, 250.0).half_rays.tolist() == [3, 2]
    w = rg.llsd_window(r, 0.5, 125.0, azimuthal_width_m=5000.0, range_width_m=10000.0, min_half_rays=3, max_half_rays=9)
    assert w.half_rays.tolist() == [0, 0, 9, 9, 8, 8, 5, 3] and w.half_gates == 16 and w.max_half_rays == 9
    assert rg.llsd_window(r, 1.0, 2000.0).half_gates == 1                                                    # floor(0.1875 + 0.5) = 0 -> 1
    assert rg.llsd_window(np.zeros(0), 1.0, 250.0).half_rays.shape == (0,)
    for kw, match in [(dict(ray_spacing_deg=0.0), "ray_spacing_deg"), (dict(gate_spacing_m=-1.0), "gate_spacing_m"),
                      (dict(gate_spacing_m=NAN), "gate_spacing_m"), (dict(azimuthal_width_m=INF), "azimuthal_width_m"),
                      (dict(range_width_m=0.0), "range_width_m"), (dict(max_half_rays=17), "max_half_rays"),
                      (dict(max_half_rays=0), "max_half_rays"), (dict(min_half_rays=-1), "min_half_rays"),
                      (dict(min_half_rays=5, max_half_rays=4), "min_half_rays"), (dict(ranges_m=np.zeros((2, 2))), "ranges_m"),
                      (dict(ranges_m=np.array([1.0, NAN])), "ranges_m")]:
        args = dict(ranges_m=r, ray_spacing_deg=1.0, gate_spacing_m=250.0)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            rg.llsd_window(**args)


# ---- refusals of the wrappers: ValueError before the library is loaded -------------------------------------------------------------
def test_wrapper_refusals():
    v = np.zeros((2, 40, 20), np.float32)
    w = rg.llsd_window(250.0 * (1 + np.arange(20)), 1.0, 250.0)
    few = np.zeros((2, 9, 20), np.float32)
    huge = np.broadcast_to(np.float32(0), (2, 40000, 30000))
    for call, match in [
            (lambda: rg.median_filter_device(v.astype(np.float64)), "float32"),
            (lambda: rg.median_filter_device(v[0, 0]), r"\[n_sweeps, n_rays, n_gates\]"),
            (lambda: rg.median_filter_device([[1.0]]), "tensor or an ndarray"),
            (lambda: rg.median_filter_device(np.zeros((0, 3, 4), np.float32)), "at least one sweep"),
            (lambda: rg.median_filter_device(huge), "2\\^31"),
            (lambda: rg.median_filter_device(v, half_rays=3), "half_rays"), (lambda: rg.median_filter_device(v, half_gates=-1), "half_gates"),
            (lambda: rg.median_filter_device(v, half_rays=1.0), "half_rays"), (lambda: rg.median_filter_device(v, half_rays=True), "half_rays"),
            (lambda: rg.median_filter_device(v, half_rays=0, half_gates=0), "both 0"),
            (lambda: rg.median_filter_device(v, min_valid=0), "min_valid"), (lambda: rg.median_filter_device(v, min_valid=26), "min_valid"),
            (lambda: rg.median_filter_device(np.zeros((1, 4, 9), np.float32), half_rays=2), "circle of 4 rays"),
            (lambda: rg.median_filter_device(v, mask=np.zeros((2, 40, 19), np.uint8)), "mask"),
            (lambda: rg.velocity_shear_device(v.astype(np.float64), w), "float32"),
            (lambda: rg.velocity_shear_device(v[0, 0], w), r"\[n_sweeps, n_rays, n_gates\]"),
            (lambda: rg.velocity_shear_device(huge, w), "2\\^31"),
            (lambda: rg.velocity_shear_device(v, None), "ShearWindow"), (lambda: rg.velocity_shear_device(v, (1, 2, 3)), "ShearWindow"),
            (lambda: rg.velocity_shear_device(v, w._replace(half_rays=w.half_rays.astype(np.int64))), "half_rays must be int32"),
            (lambda: rg.velocity_shear_device(v, w._replace(half_rays=w.half_rays[:5])), "half_rays must be int32 \\[20\\]"),
            (lambda: rg.velocity_shear_device(v, w._replace(az_scale=w.az_scale.astype(np.float32))), "az_scale must be float64"),
            (lambda: rg.velocity_shear_device(v, w._replace(az_scale=list(w.az_scale))), "az_scale"),
            (lambda: rg.velocity_shear_device(v, w._replace(max_half_rays=0)), "max_half_rays"),
            (lambda: rg.velocity_shear_device(v, w._replace(max_half_rays=17)), "max_half_rays"),
            (lambda: rg.velocity_shear_device(v, w._replace(half_gates=0)), "half_gates"),
            (lambda: rg.velocity_shear_device(v, w._replace(half_gates=17)), "half_gates"),
            (lambda: rg.velocity_shear_device(v, w._replace(half_gates=2.0)), "half_gates"),
            (lambda: rg.velocity_shear_device(v, w._replace(range_scale=INF)), "range_scale"),
            (lambda: rg.velocity_shear_device(v, w._replace(range_scale=NAN)), "range_scale"),
            (lambda: rg.velocity_shear_device(v, w._replace(range_scale="x")), "range_scale"),
            (lambda: rg.velocity_shear_device(few, w), "does not fit a circle of 9 rays"),
            (lambda: rg.velocity_shear_device(v[:, :32], w), "does not fit a circle of 32 rays"),
            (lambda: rg.velocity_shear_device(v, w, min_valid=2), "min_valid"), (lambda: rg.velocity_shear_device(v, w, min_valid=1090), "min_valid"),
            (lambda: rg.velocity_shear_device(v, w, min_valid=6.0), "min_valid"),
            (lambda: rg.velocity_shear_device(v, w, min_fraction=-0.1), "min_fraction"), (lambda: rg.velocity_shear_device(v, w, min_fraction=1.5), "min_fraction"),
            (lambda: rg.velocity_shear_device(v, w, min_fraction=NAN), "min_fraction"), (lambda: rg.velocity_shear_device(v, w, min_fraction=None), "min_fraction"),
            (lambda: rg.velocity_shear_device(v, w, want=("vorticity",)), "want"), (lambda: rg.velocity_shear_device(v, w, want="velocity"), "want"),
            (lambda: rg.velocity_shear_device(v, w, want=()), "at least one"), (lambda: rg.velocity_shear_device(v, w, want=("count",)), "at least one"),
            (lambda: rg.velocity_shear_device(v, w, mask=np.zeros((40, 20), np.uint8)), "mask"),
            (lambda: rg.azimuthal_shear_device(v, w, median=(3, 1)), "half_rays"), (lambda: rg.azimuthal_shear_device(v, w, median=(0, 0)), "both 0"),
            (lambda: rg.azimuthal_shear_device(v, w, median=1), "median must be"), (lambda: rg.azimuthal_shear_device(v, w, median=(1, 1, 1)), "median must be"),
            (lambda: rg.azimuthal_shear_device(few, w), "does not fit a circle"),
            (lambda: rg.azimuthal_shear_device(v, w, min_valid=0), "min_valid"),
            (lambda: rg.velocity_shear(v.astype(np.float64), w), "float32"),
            (lambda: rg.velocity_shear(v, w, want=("shear",)), "want")]:
        with pytest.raises(ValueError, match=match):
            call()
    # the circle only has to hold the window under wrap_rays
    assert shear._check_window(w, (2, 9, 20), False).max_half_rays == 16
    assert shear._check_fit(6, 0.5, ("count", "velocity")) == (6, 32768, ("count", "velocity"))
    assert shear._check_fit(3, 1.0, ("velocity",))[1] == 65536 and shear._check_fit(3, 0.00001, ("velocity",))[1] == 1


# ---- refusals of the C ABI: each returns before any HIP call ---------------------------------------------------------------------
def median_args(**kw):
    a = dict(vel=P, mask=2 * P, S=2, R=40, G=100, half_rays=1, half_gates=1, wrap=1, min_valid=1, centre=1, out=4 * P)
    a.update(kw)
    return (a["vel"], a["mask"], a["S"], a["R"], a["G"], a["half_rays"], a["half_gates"], a["wrap"], a["min_valid"], a["centre"], a["out"],
            None)


def llsd_args(**kw):
    a = dict(vel=P, mask=2 * P, S=2, R=40, G=100, half_rays=3 * P, az_scale=4 * P, max_half_rays=16, half_gates=2, range_scale=1e-7,
             wrap=1, min_valid=6, q16=32768, centre=0, az_shear=5 * P, divergence=6 * P, vel_s=7 * P, count=8 * P)
    a.update(kw)
    return (a["vel"], a["mask"], a["S"], a["R"], a["G"], a["half_rays"], a["az_scale"], a["max_half_rays"], a["half_gates"],
            a["range_scale"], a["wrap"], a["min_valid"], a["q16"], a["centre"], a["az_shear"], a["divergence"], a["vel_s"], a["count"], None)


SIZES = [(dict(S=0), "S and R must be at least 1, got 0 and 40"), (dict(R=0), "S and R must be at least 1, got 2 and 0"),
         (dict(G=-1), "G must not be negative, got -1"), (dict(S=2, R=32768, G=32768), "2 sweeps of 32768 x 32768 are 2^31 gates or more")]
N = 2 * 40 * 100                             # gates of the default volume: 32000 bytes of float32, 8000 of mask, 16000 of count

REFUSALS = {
    "rg_polar_median_f32": (median_args, SIZES + [
        (dict(vel=None), "null pointer"), (dict(out=None), "null pointer"),
        (dict(half_rays=3), "half_rays and half_gates must lie in 0 .. 2, got 3 and 1"),
        (dict(half_gates=-1), "half_rays and half_gates must lie in 0 .. 2, got 1 and -1"),
        (dict(half_rays=0, half_gates=0), "half_rays and half_gates are both 0"),
        (dict(R=4, half_rays=2), "a window of 5 rays does not fit a circle of 4 rays"),
        (dict(R=2), "a window of 3 rays does not fit a circle of 2 rays"),
        (dict(min_valid=0), "min_valid must lie in 1 .. 25, got 0"), (dict(min_valid=26), "min_valid must lie in 1 .. 25, got 26"),
        (dict(out=P), "out overlaps vel"), (dict(out=P + 4 * N - 4), "out overlaps vel"), (dict(out=P - 4 * N + 4), "out overlaps vel"),
        (dict(out=2 * P + N - 1), "out overlaps mask")]),
    "rg_velocity_llsd_f32": (llsd_args, SIZES + [
        (dict(vel=None), "null pointer"), (dict(half_rays=None), "null pointer"), (dict(az_scale=None), "null pointer"),
        (dict(az_shear=None, divergence=None, vel_s=None), "none of az_shear, divergence and vel_s is asked for"),
        (dict(max_half_rays=0), "max_half_rays must lie in 1 .. 16, got 0"), (dict(max_half_rays=17), "max_half_rays must lie in 1 .. 16, got 17"),
        (dict(half_gates=0), "half_gates must lie in 1 .. 16, got 0"), (dict(half_gates=17), "half_gates must lie in 1 .. 16, got 17"),
        (dict(R=32), "a window of 33 rays does not fit a circle of 32 rays"),
        (dict(R=4, max_half_rays=2), "a window of 5 rays does not fit a circle of 4 rays"),
        (dict(min_valid=2), "min_valid must lie in 3 .. 1089, got 2"), (dict(min_valid=1090), "min_valid must lie in 3 .. 1089, got 1090"),
        (dict(q16=-1), "min_fraction_q16 must lie in 0 .. 65536, got -1"), (dict(q16=65537), "min_fraction_q16 must lie in 0 .. 65536, got 65537"),
        (dict(range_scale=INF), "range_scale must be finite, got inf"), (dict(range_scale=NAN), "range_scale must be finite, got nan"),
        (dict(az_shear=P), "az_shear overlaps vel"), (dict(divergence=2 * P + N - 1), "divergence overlaps mask"),
        (dict(vel_s=3 * P + 396), "vel_s overlaps half_rays"), (dict(count=4 * P + 792), "count overlaps az_scale"),
        (dict(count=P - 2 * N + 2), "count overlaps vel"), (dict(az_shear=6 * P + 4), "az_shear overlaps divergence"),
        (dict(divergence=7 * P), "divergence overlaps vel_s"), (dict(vel_s=8 * P + 2 * N - 4), "vel_s overlaps count"),
        (dict(az_shear=None, divergence=None, vel_s=8 * P), "vel_s overlaps count")]),
}
CASES = [(name, kw, message) for name, (_, cases) in REFUSALS.items() for kw, message in cases]


@pytest.mark.parametrize("name,kw,message", CASES)
def test_refusals_name_the_function_and_the_reason(name, kw, message):
    lib = rg.load_library(require_device=False)
    assert getattr(lib, name)(*REFUSALS[name][0](**kw)) == _native.RG_EINVAL
    assert lib.rg_last_error().decode() == f"{name}: {message}"


def test_alignment_and_nothing_to_do():
    lib = rg.load_library(require_device=False)
    assert lib.rg_velocity_llsd_f32(*llsd_args(az_scale=4 * P + 4)) == _native.RG_EALIGN
    assert lib.rg_last_error().decode() == "rg_velocity_llsd_f32: az_scale must be 8-byte aligned"
    # G == 0 returns RG_OK before any launch, whatever coincides: every array is empty.  Without wrap a single ray will do.
    assert lib.rg_polar_median_f32(*median_args(G=0, out=P)) == _native.RG_OK
    assert lib.rg_polar_median_f32(*median_args(G=0, mask=None, R=1, wrap=0)) == _native.RG_OK
    assert lib.rg_velocity_llsd_f32(*llsd_args(G=0, az_shear=P, divergence=None, vel_s=None, count=None)) == _native.RG_OK
    assert lib.rg_velocity_llsd_f32(*llsd_args(G=0, R=1, wrap=0, mask=None)) == _native.RG_OK


# ---- the two restatements check each other ---------------------------------------------------------------------------------------
def _tiny(seed, S, R, G):
    rng = np.random.default_rng(seed)
    vel = (np.round(rng.normal(0.0, 9.0, (S, R, G)) * 32.0) / 32.0).astype(np.float32)
    vel[rng.random(vel.shape) < 0.2] = np.nan
    vel[0, 0, 0] = np.inf
    vel[0, R - 1, G - 1] = 20000.0
    mask = (rng.random(vel.shape) < 0.1).astype(np.uint8) * np.uint8(200)
    return vel, mask


@pytest.mark.parametrize("seed,S,R,G,hg,wrap,centre", [(1, 2, 9, 11, 2, 1, 0), (2, 1, 9, 7, 1, 0, 1), (3, 2, 7, 4, 3, 1, 1), (4, 1, 1, 9, 2, 0, 0),
                                                       (5, 1, 5, 1, 1, 1, 0), (6, 2, 12, 6, 2, 0, 0)])
def test_vectorised_llsd_equals_the_naive_one(seed, S, R, G, hg, wrap, centre):
    vel, mask = _tiny(seed, S, R, G)
    rng = np.random.default_rng(seed + 50)
    max_half = min(4, (R - 1) // 2) if wrap else 4
    assert max_half >= 1 and (not wrap or 2 * max_half + 1 <= R)
    half_rays = rng.integers(-1, 7, G).astype(np.int32)
    az_scale = rng.uniform(1e-7, 1e-5, G)
    args = (vel, mask, half_rays, az_scale, max_half, hg, 3.1e-8, wrap, 3, 9000, centre)
    fast, slow = so.llsd(*args), so.llsd_naive(*args)
    assert np.array_equal(fast.count, slow.count)
    for a, b in zip(fast[:3], slow[:3]):
        assert np.array_equal(so.bits(a), so.bits(b))
    assert (~np.isnan(fast.az_shear)).any() or R == 1 or G == 1


def test_vectorised_llsd_equals_the_naive_one_on_tiny_cuts_of_the_scenes():
    for name in ("seams_wrap", "thresholds_centre", "degenerate_diagonal", "plane"):
        s = dict(ss.scenes()[name])
        R = min(s["vel"].shape[1], 37 if s["wrap"] else 9)
        s["vel"] = s["vel"][:1, :R, :24]
        s["mask"] = None if s["mask"] is None else s["mask"][:1, :R, :24]
        s["half_rays"], s["az_scale"] = s["half_rays"][:24], s["az_scale"][:24]
        if name == "seams_wrap":                                        # 37 rays x 24 gates x windows of 33 x 7 is the most a loop should do
            s["vel"], s["mask"] = s["vel"][:, :, :12], s["mask"][:, :, :12]
            s["half_rays"], s["az_scale"] = s["half_rays"][:12] + np.int32(14), s["az_scale"][:12]
        fast, slow = so.llsd(*ss.llsd_args(s)), so.llsd_naive(*ss.llsd_args(s))
        assert np.array_equal(fast.count, slow.count), name
        for a, b in zip(fast[:3], slow[:3]):
            assert np.array_equal(so.bits(a), so.bits(b)), name


def test_vectorised_median_equals_the_naive_one():
    vel, mask = ss.median_data()
    for hr, hg, wrap, min_valid, centre in ss.median_cases():
        fast, slow = so.median(vel, mask, hr, hg, wrap, min_valid, centre), so.median_naive(vel, mask, hr, hg, wrap, min_valid, centre)
        assert np.array_equal(so.bits(fast), so.bits(slow)), (hr, hg, wrap, min_valid, centre)
    assert np.array_equal(so.bits(so.median(vel, None, 1, 2, 1, 1, 0)), so.bits(so.median_naive(vel, None, 1, 2, 1, 1, 0)))
