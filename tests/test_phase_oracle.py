"""CPU-side checks of the polar-domain phase processing (no GPU needed): the third header against ``_native.PHASE_SIGNATURES``,
the exports, the refusals of the wrappers and of the three entry points (all of which return before any HIP call), and the
properties of the NumPy restatement that follow from the contract."""
import ctypes
import os
import re

import numpy as np
import pytest

import radar_processor_amd as rg
from radar_processor_amd import _native, phase

import phase_oracle as po
import phase_scenes as ps

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "radargrid_phase.h")
NAMES = {"rg_phidp_unfold_f32", "rg_phidp_fit_f32", "rg_attenuation_phidp_f32"}
P = 1 << 16                                  # an aligned address that is never dereferenced
NAN, INF = float("nan"), float("inf")


# ---- the third header ------------------------------------------------------------------------------------------------------------
def _declared():
    """name -> [(C type, argument name)] of every function the header declares."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"^int\s+(rg_\w+)\s*\(([^;]*)\);", text, flags=re.M):
        out[name] = [tuple(a.strip().rsplit(" ", 1)) for a in args.replace("\n", " ").split(",")]
    return out


def _ctype(ctype, name):
    if name.endswith("_host"):
        return {"const double*": ctypes.POINTER(ctypes.c_double), "const int32_t*": ctypes.POINTER(ctypes.c_int32)}[ctype]
    if ctype.endswith("*") or ctype == "rg_stream_t":
        return ctypes.c_void_p
    return {"int32_t": ctypes.c_int32, "double": ctypes.c_double}[ctype]


def test_header_and_table_mirror_each_other_one_to_one():
    declared = _declared()
    assert set(declared) == set(_native.PHASE_SIGNATURES) == NAMES
    assert not NAMES & set(_native.SIGNATURES) and not NAMES & set(_native.ENSEMBLE_SIGNATURES)
    lib = rg.load_library(require_device=False)
    raw = ctypes.CDLL(_native.LIB_PATH)
    for name, args in declared.items():
        restype, argtypes = _native.PHASE_SIGNATURES[name]
        assert restype is ctypes.c_int32 and argtypes == [_ctype(*a) for a in args], name
        assert args[-1] == ("rg_stream_t", "stream"), f"{name}: the stream comes last"
        assert hasattr(raw, name), f"{name} declared in the header but not exported"
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    header = open(HEADER).read()
    assert '#include "radargrid_hip.h"' in header
    for macro in ("RG_PHASE_MAX_GATES", "RG_PHASE_MAX_CLASSES", "RG_PHASE_MAX_HALF_WINDOW", "RG_PHASE_MAX_ABS_PHI",
                  "RG_PHASE_MAX_WORKGROUPS"):
        assert re.search(r"#define %s %d\b" % (macro, getattr(_native, macro)), header), macro
    assert lib.rg_version() == _native.ABI_VERSION == 104


def test_the_new_unit_and_header_are_part_of_the_build():
    from radar_processor_amd import build
    assert ("rg_phase.hip", []) in build.SOURCES and build.SOURCES[-1] == ("rg_warp.hip", [])
    assert build.PUBLIC_HEADERS == ["radargrid_hip.h", "radargrid_ensemble.h", "radargrid_phase.h"]
    assert HEADER in build.sources_and_headers()


def test_exports():
    names = ["unfold_phidp_device", "fit_phidp_device", "correct_attenuation_device", "process_phase_device", "process_phase",
             "ATTENUATION_COEFFICIENTS", "PhaseFit", "AttenuationCorrection", "PhaseProducts"]
    for name in names:
        assert name in rg.__all__ and getattr(rg, name) is getattr(phase, name), name
    assert rg.PhaseFit._fields == ("kdp", "phidp", "count")
    assert rg.AttenuationCorrection._fields == ("dbz", "zdr", "pia", "dphi")
    assert rg.PhaseProducts._fields == ("phidp_unfolded", "phidp", "kdp", "count", "dbz", "zdr", "pia", "dphi")
    assert set(rg.ATTENUATION_COEFFICIENTS) == {"S", "C", "X"}
    a = [rg.ATTENUATION_COEFFICIENTS[b] for b in "SCX"]
    assert all(0 < beta < alpha < 1 for alpha, beta in a) and a[0][0] < a[1][0] < a[2][0]      # attenuation grows with frequency
    assert phase.scale_for(240.0) == 500.0 / (65536.0 * 240.0)


# ---- refusals of the wrappers: ValueError before the library is loaded -------------------------------------------------------------
def test_wrapper_refusals():
    f = np.zeros((3, 20), np.float32)
    for call, match in [
            (lambda: rg.unfold_phidp_device(f.astype(np.float64)), "float32"),
            (lambda: rg.unfold_phidp_device(f[0]), r"\[n_rays, n_gates\]"),
            (lambda: rg.unfold_phidp_device(np.zeros((0, 4), np.float32)), "at least one ray"),
            (lambda: rg.unfold_phidp_device(np.zeros((1, 32769), np.float32)), "32768 gates"),
            (lambda: rg.unfold_phidp_device([[1.0]]), "tensor or an ndarray"),
            (lambda: rg.unfold_phidp_device(f, mask=np.zeros((3, 19), np.uint8)), "mask"),
            (lambda: rg.unfold_phidp_device(f, wrap=0.0), "wrap"), (lambda: rg.unfold_phidp_device(f, wrap=NAN), "wrap"),
            (lambda: rg.unfold_phidp_device(f, wrap=1e39), "wrap"),
            (lambda: rg.fit_phidp_device(f, 0.0), "gate_spacing_m"), (lambda: rg.fit_phidp_device(f, INF), "gate_spacing_m"),
            (lambda: rg.fit_phidp_device(f, 240.0, half_window=0), "half_window"),
            (lambda: rg.fit_phidp_device(f, 240.0, half_window=256), "half_window"),
            (lambda: rg.fit_phidp_device(f, 240.0, half_window=2.5), "half_window"),
            (lambda: rg.fit_phidp_device(f, 240.0, half_window=(3, 4)), "one integer per class"),
            (lambda: rg.fit_phidp_device(f, 240.0, half_window=(3, 4), dbz_edges=(30.0,)), "without dbz"),
            (lambda: rg.fit_phidp_device(f, 240.0, half_window=(3, 4, 5), dbz=f, dbz_edges=(30.0, 20.0)), "ascend"),
            (lambda: rg.fit_phidp_device(f, 240.0, half_window=3, dbz=f, dbz_edges=(1.0, 2.0, 3.0, 4.0)), "at most 3 edges"),
            (lambda: rg.fit_phidp_device(f, 240.0, dbz=f, dbz_edges=(NAN,)), "edge"),
            (lambda: rg.fit_phidp_device(f, 240.0, dbz=f.astype(np.float64)), "dbz must be float32"),
            (lambda: rg.fit_phidp_device(f, 240.0, min_valid=1), "min_valid"),
            (lambda: rg.fit_phidp_device(f, 240.0, min_valid=512), "min_valid"),
            (lambda: rg.correct_attenuation_device(f, f[:, :5], alpha=0.1, beta=0.0), "dbz"),
            (lambda: rg.correct_attenuation_device(f, None, alpha=0.1, beta=0.0), "dbz is required"),
            (lambda: rg.correct_attenuation_device(f, f, alpha=-0.1, beta=0.0), "alpha"),
            (lambda: rg.correct_attenuation_device(f, f, alpha=0.1, beta=NAN), "beta"),
            (lambda: rg.correct_attenuation_device(f, f, alpha=0.1, beta=0.0, max_dphi=0.0), "max_dphi"),
            (lambda: rg.correct_attenuation_device(f, f, alpha=0.1, beta=0.0, phi0=np.zeros(4, np.float32)), "phi0"),
            (lambda: rg.correct_attenuation_device(f, f, alpha=0.1, beta=0.0, phi0=np.zeros(3)), "phi0"),
            (lambda: rg.correct_attenuation_device(f, f, alpha=0.1, beta=0.0, zdr=f.T), "zdr"),
            (lambda: rg.process_phase_device(f, f, 240.0, band="K"), "band"),
            (lambda: rg.process_phase_device(f, f, -1.0), "gate_spacing_m"),
            (lambda: rg.process_phase(f, f, 240.0, mask=np.zeros((2, 20), np.uint8)), "mask")]:
        with pytest.raises(ValueError, match=match):
            call()
    with pytest.raises(TypeError):
        rg.correct_attenuation_device(f, f)                                   # alpha and beta have no default
    # more rays than one launch holds (no memory behind these views): refused before the library is loaded
    many, more = np.broadcast_to(np.float32(0.0), (2 ** 24, 100)), np.broadcast_to(np.float32(0.0), (2 ** 26 - 3, 1))
    for call, match in [(lambda: rg.fit_phidp_device(many, 240.0), "split the volume by rays"),
                        (lambda: rg.process_phase_device(many, many, 240.0), "split the volume by rays"),
                        (lambda: rg.unfold_phidp_device(more), "at most 67108860 rays"),
                        (lambda: rg.correct_attenuation_device(more, more, alpha=0.1, beta=0.0), "at most 67108860 rays")]:
        with pytest.raises(ValueError, match=match):
            call()


# ---- refusals of the C ABI: each returns before any HIP call ---------------------------------------------------------------------
def unfold_args(**kw):
    a = dict(phidp=P, mask=2 * P, R=4, G=100, wrap=360.0, out=4 * P, folds=5 * P)
    a.update(kw)
    return a["phidp"], a["mask"], a["R"], a["G"], a["wrap"], a["out"], a["folds"], None


def fit_args(**kw):
    a = dict(phi=P, R=4, G=100, dbz=2 * P, edges=[10.0, 30.0], half=[9, 5, 3], n_classes=None, min_valid=3, centre_only=0,
             scale=1.0, kdp=4 * P, phi_s=5 * P, count=6 * P)
    a.update(kw)
    n = len(a["half"]) if a["n_classes"] is None else a["n_classes"]
    edges = None if a["edges"] is None else (ctypes.c_double * max(len(a["edges"]), 1))(*a["edges"])
    half = None if a["half"] is None else (ctypes.c_int32 * max(len(a["half"]), 1))(*a["half"])
    return (a["phi"], a["R"], a["G"], a["dbz"], edges, half, n, a["min_valid"], a["centre_only"], a["scale"], a["kdp"],
            a["phi_s"], a["count"], None)


def attenuation_args(**kw):
    a = dict(phi_s=P, phi0=2 * P, R=4, G=100, alpha=0.08, beta=0.02, max_dphi=360.0, dbz=3 * P, zdr=4 * P, dbz_out=5 * P,
             zdr_out=6 * P, pia=7 * P, dphi=8 * P)
    a.update(kw)
    return (a["phi_s"], a["phi0"], a["R"], a["G"], a["alpha"], a["beta"], a["max_dphi"], a["dbz"], a["zdr"], a["dbz_out"],
            a["zdr_out"], a["pia"], a["dphi"], None)


SIZES = [(dict(R=0), "R must be at least 1, got 0"), (dict(G=-1), "G must lie in 0 .. 32768, got -1"),
         (dict(G=32769), "G must lie in 0 .. 32768, got 32769"), (dict(R=65536, G=32768), "R * G must stay below 2^31, got 65536 x 32768")]
REFUSALS = {
    "rg_phidp_unfold_f32": (unfold_args, SIZES + [
        (dict(phidp=None), "null pointer"), (dict(out=None), "null pointer"),
        (dict(R=2 ** 26 - 3, G=1), "67108861 rays of 1 gates take 16777216 workgroups, one launch holds 16777215"),
        (dict(wrap=0.0), "wrap must be finite and positive with a finite positive float32 half, got 0"),
        (dict(wrap=-360.0), "wrap must be finite and positive with a finite positive float32 half, got -360"),
        (dict(wrap=NAN), "wrap must be finite and positive with a finite positive float32 half, got nan"),
        (dict(wrap=INF), "wrap must be finite and positive with a finite positive float32 half, got inf"),
        (dict(wrap=1e-60), "wrap must be finite and positive with a finite positive float32 half, got 1e-60"),
        (dict(out=P + 4), "out overlaps phidp"), (dict(out=2 * P + 399), "out overlaps mask"), (dict(folds=P), "folds overlaps phidp"),
        (dict(folds=2 * P), "folds overlaps mask"), (dict(folds=4 * P + 1596), "out overlaps folds"),
        (dict(out=P, folds=P), "out overlaps folds")]),
    "rg_phidp_fit_f32": (fit_args, SIZES + [
        (dict(phi=None), "null pointer"), (dict(half=None, n_classes=1), "null pointer"), (dict(edges=None), "null pointer"),
        (dict(kdp=None, phi_s=None), "kdp and phi_s are both NULL"),
        (dict(R=2 ** 24, G=100), "16777216 rays of 100 gates take 16777216 workgroups, one launch holds 16777215"),
        (dict(half=[], n_classes=0), "n_classes must lie in 1 .. 4, got 0"), (dict(n_classes=5), "n_classes must lie in 1 .. 4, got 5"),
        (dict(half=[9, 0, 3]), "half-window 1 must lie in 1 .. 255, got 0"),
        (dict(half=[256, 5, 3]), "half-window 0 must lie in 1 .. 255, got 256"),
        (dict(edges=[10.0, NAN]), "edge 1 is not finite"), (dict(edges=[INF, 30.0]), "edge 0 is not finite"),
        (dict(edges=[30.0, 10.0]), "the edges must ascend, edge 1 does not"),
        (dict(min_valid=1), "min_valid must lie in 2 .. 511, got 1"), (dict(min_valid=512), "min_valid must lie in 2 .. 511, got 512"),
        (dict(scale=NAN), "scale is not finite"), (dict(scale=INF), "scale is not finite"),
        (dict(kdp=P), "kdp overlaps phi"), (dict(phi_s=2 * P + 396), "phi_s overlaps dbz"), (dict(count=P + 1599), "count overlaps phi"),
        (dict(phi_s=4 * P), "kdp overlaps phi_s"), (dict(count=5 * P + 1598), "phi_s overlaps count")]),
    "rg_attenuation_phidp_f32": (attenuation_args, SIZES + [
        (dict(phi_s=None), "null pointer"), (dict(dbz=None), "null pointer"), (dict(dbz_out=None), "null pointer"),
        (dict(R=2 ** 26, G=2), "67108864 rays of 2 gates take 16777216 workgroups, one launch holds 16777215"),
        (dict(zdr=None), "zdr and zdr_out come together or not at all"), (dict(zdr_out=None), "zdr and zdr_out come together or not at all"),
        (dict(alpha=-0.1), "alpha and beta must be finite and not negative, got -0.1 and 0.02"),
        (dict(beta=NAN), "alpha and beta must be finite and not negative, got 0.08 and nan"),
        (dict(alpha=INF), "alpha and beta must be finite and not negative, got inf and 0.02"),
        (dict(max_dphi=0.0), "max_dphi must be finite and positive in float32, got 0"),
        (dict(max_dphi=INF), "max_dphi must be finite and positive in float32, got inf"),
        (dict(max_dphi=NAN), "max_dphi must be finite and positive in float32, got nan"),
        (dict(dbz_out=P), "dbz_out overlaps phi_s"), (dict(dbz_out=3 * P + 4), "dbz_out overlaps dbz"),
        (dict(dbz_out=2 * P + 12), "dbz_out overlaps phi0"), (dict(zdr_out=3 * P), "zdr_out overlaps dbz"),
        (dict(zdr_out=4 * P + 396), "zdr_out overlaps zdr"), (dict(pia=3 * P), "pia overlaps dbz"), (dict(dphi=P), "dphi overlaps phi_s"),
        (dict(pia=5 * P), "dbz_out overlaps pia"), (dict(dphi=7 * P + 1596), "pia overlaps dphi"),
        (dict(dbz_out=3 * P, zdr_out=3 * P), "dbz_out overlaps zdr_out")]),
}
CASES = [(name, kw, message) for name, (_, cases) in REFUSALS.items() for kw, message in cases]


@pytest.mark.parametrize("name,kw,message", CASES)
def test_refusals_name_the_function_and_the_reason(name, kw, message):
    lib = rg.load_library(require_device=False)
    assert getattr(lib, name)(*REFUSALS[name][0](**kw)) == _native.RG_EINVAL
    assert lib.rg_last_error().decode() == f"{name}: {message}"


def test_nothing_to_do_and_the_allowed_in_place_uses_are_ok_without_a_launch():
    """G == 0 returns RG_OK before any launch, whatever coincides: every array is empty."""
    lib = rg.load_library(require_device=False)
    assert lib.rg_phidp_unfold_f32(*unfold_args(G=0, out=P, folds=P)) == _native.RG_OK
    assert lib.rg_phidp_fit_f32(*fit_args(G=0, kdp=P)) == _native.RG_OK
    assert lib.rg_phidp_fit_f32(*fit_args(G=0, edges=None, half=[7], dbz=None, count=None, kdp=None)) == _native.RG_OK
    assert lib.rg_attenuation_phidp_f32(*attenuation_args(G=0, zdr=None, zdr_out=None, pia=None, dphi=None, phi0=None)) == _native.RG_OK


# ---- what follows from the contract ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing,slope,L", [(240.0, 0.25, 15), (125.0, 0.75, 3), (1000.0, -0.5, 255), (60.0, 2.0 ** -10, 40)])
def test_an_exact_ramp_returns_itself_and_its_slope(spacing, slope, L):
    """Values that float32 holds exactly and the 2^-16 fixed point too: the fit is exact up to the float64 roundings, so phi_s
    is the ramp bit for bit.  KDP: within the worst-case slope error of a 2^-17 degree quantisation, sum |j - jbar| /
    sum (j - jbar)^2 <= 2 times it, 2^-16 degrees per gate, times 500 / gate_spacing_m."""
    G = 300
    phi = (100.0 + slope * np.arange(G)).astype(np.float32)[None, :]
    assert np.array_equal(phi.astype(np.float64), 100.0 + slope * np.arange(G)[None, :])
    f = po.fit(phi, phase.scale_for(spacing), half_window=(L,), min_valid=2)
    assert np.array_equal(po.bits(f.phi_s), po.bits(phi))
    assert np.abs(f.kdp.astype(np.float64) - slope * 500.0 / spacing).max() <= 2.0 ** -16 * 500.0 / spacing
    noisy = (phi.astype(np.float64) + np.random.default_rng(L).uniform(-2.0 ** -17, 2.0 ** -17, phi.shape))
    g = po.fit(noisy.astype(np.float32), phase.scale_for(spacing), half_window=(L,), min_valid=2)
    assert np.abs(g.kdp.astype(np.float64) - slope * 500.0 / spacing).max() <= 2.0 ** -16 * 500.0 / spacing


@pytest.mark.parametrize("wrap", [360.0, 180.0])
def test_unfold_restores_a_rewrapped_ramp(wrap):
    G = 520
    truth = ((-170.0 + 2.5 * np.arange(G)) * (wrap / 360.0))[None, :]                         # exact in float32, steps << wrap / 2
    wrapped = (truth - wrap * np.floor((truth + 0.5 * wrap) / wrap)).astype(np.float32)
    assert wrapped.min() >= -0.5 * wrap and wrapped.max() < 0.5 * wrap and truth.max() > 3 * wrap
    out, folds = po.unfold(wrapped, None, wrap)
    assert np.array_equal(out, truth.astype(np.float32)) and folds.max() >= 3
    mask = (np.arange(G) % 7 == 3).astype(np.uint8)[None, :]
    out, _ = po.unfold(wrapped, mask, wrap)
    assert np.array_equal(out[mask == 0], truth.astype(np.float32)[mask == 0]) and np.isnan(out[mask != 0]).all()


def test_dphi_never_decreases_and_never_leaves_its_range():
    for s in ps.attenuation_scenes().values():
        a = po.attenuation(s.phi_s, s.dbz, alpha=s.alpha, beta=s.beta, max_dphi=s.max_dphi, zdr=s.zdr, phi0=s.phi0)
        assert (np.diff(a.dphi, axis=1) >= 0).all() and (a.dphi >= 0).all() and (a.dphi <= np.float32(s.max_dphi)).all()
        assert not np.signbit(a.dphi).any() and a.dphi.dtype == np.float32
        assert (np.isnan(a.dbz) == np.isnan(s.dbz)).all()


@pytest.mark.parametrize("name", ["fit_5x65", "fit_1x129", "fit_5x200", "l255", "sparse", "pairs", "limits", "gaps_centre"])
def test_the_fit_does_not_depend_on_how_the_sums_are_formed(name):
    s = ps.fit_scenes()[name]
    kw = dict(half_window=s.half_window, min_valid=s.min_valid, dbz=s.dbz, edges=s.edges, centre_only=s.centre_only)
    a, b = po.fit(s.phi, phase.scale_for(s.spacing), **kw), po.fit_direct(s.phi, phase.scale_for(s.spacing), **kw)
    for x, y in zip(a, b):
        assert np.array_equal(po.bits(x), po.bits(y))
