"""CPU-side checks of the hydrometeor classification (no GPU needed): the sixth header against ``_native.HYDRO_SIGNATURES``, the
macros, the build lists, the exports, the refusals of the entry points (all of which return before any HIP call) and of the
wrappers, the vectorised restatement against the naive one, ``MembershipTable`` and ``beam_temperature`` against values worked out
by hand, and the preset on a handful of archetypal signatures."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import radar_processor_amd as rg
from radar_processor_amd import _native, hydrometeor

import hydro_oracle as ho
import hydro_scenes as hs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "radargrid_hydro.h")
NAMES = {"rg_polar_texture_f32", "rg_fuzzy_classify_f32"}
MACROS = ("RG_HYDRO_TEXTURE_SHIFT", "RG_HYDRO_MAX_ABS", "RG_HYDRO_MAX_HALF_GATES", "RG_HYDRO_TEXTURE_TILE", "RG_HYDRO_MAX_VARS",
          "RG_HYDRO_MAX_CLASSES", "RG_HYDRO_MAX_BINS", "RG_HYDRO_MAX_CELLS", "RG_HYDRO_UNCLASSIFIED")
P = 1 << 20                                  # an aligned address that is never dereferenced
NAN, INF = float("nan"), float("inf")


# ---- the sixth header ------------------------------------------------------------------------------------------------------------
def _declared():
    """name -> (return type, [(C type, argument name)]) of every function the header declares."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"^(int|int64_t)\s+(rg_\w+)\s*\(([^;]*)\);", text, flags=re.M):
        out[name] = (ret, [tuple(a.strip().rsplit(" ", 1)) for a in args.replace("\n", " ").split(",")])
    return out


def _ctype(ctype, name):
    if name.endswith("_host"):                   # read on the host: a typed pointer
        return {"const float* const*": ctypes.POINTER(ctypes.c_void_p), "const int32_t*": ctypes.POINTER(ctypes.c_int32),
                "const double*": ctypes.POINTER(ctypes.c_double)}[ctype]
    if ctype.endswith("*") or ctype == "rg_stream_t":
        return ctypes.c_void_p
    return {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}[ctype]


def test_header_and_table_mirror_each_other_one_to_one():
    declared = _declared()
    assert set(declared) == set(_native.HYDRO_SIGNATURES) == NAMES
    for table in (_native.SIGNATURES, _native.ENSEMBLE_SIGNATURES, _native.PHASE_SIGNATURES, _native.VELOCITY_SIGNATURES,
                  _native.SHEAR_SIGNATURES):
        assert not NAMES & set(table)
    lib = rg.load_library(require_device=False)
    raw = ctypes.CDLL(_native.LIB_PATH)
    for name, (ret, args) in declared.items():
        restype, argtypes = _native.HYDRO_SIGNATURES[name]
        assert restype is {"int": ctypes.c_int32, "int64_t": ctypes.c_int64}[ret], name
        assert argtypes == [_ctype(*a) for a in args], name
        assert args[-1] == ("rg_stream_t", "stream"), f"{name}: the stream comes last"
        assert hasattr(raw, name), f"{name} declared in the header but not exported"
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert [a[1] for a in declared["rg_fuzzy_classify_f32"][1] if a[1].endswith("_host")] == ["vars_host", "kind_host", "edges_host",
                                                                                              "weights_host"]
    header = open(HEADER).read()
    assert '#include "radargrid_hip.h"' in header and '#include "radargrid_phase.h"' in header
    for macro in MACROS:
        assert re.search(r"#define %s %d\b" % (macro, getattr(_native, macro)), header), macro
    assert (_native.RG_HYDRO_TEXTURE_SHIFT, _native.RG_HYDRO_MAX_ABS, _native.RG_HYDRO_MAX_HALF_GATES, _native.RG_HYDRO_MAX_VARS,
            _native.RG_HYDRO_MAX_CLASSES, _native.RG_HYDRO_MAX_BINS, _native.RG_HYDRO_MAX_CELLS) == (10, 8192, 63, 8, 16, 32, 1024)
    assert _native.RG_HYDRO_MAX_CELLS * 48 == 48 * 1024 and hs.TILE == _native.RG_HYDRO_TEXTURE_TILE
    assert "2^60" in header                                               # the bound of N * Sqq and Sq^2 is stated
    assert lib.rg_version() == _native.ABI_VERSION == 104


def test_the_new_unit_and_header_are_part_of_the_build_and_the_pinned_lists_are_unchanged():
    from radar_processor_amd import build
    assert build.SOURCES[-1] == ("rg_warp.hip", [])
    at = build.SOURCES.index(("rg_hydro.hip", []))
    assert build.SOURCES[at - 1] == ("rg_shear.hip", []) and build.SOURCES[at + 1] == ("rg_warp.hip", [])
    assert build.SOURCES.index(("rg_shear.hip", [])) == build.SOURCES.index(("rg_velocity.hip", [])) + 1
    assert build.PUBLIC_HEADERS == ["radargrid_hip.h", "radargrid_ensemble.h", "radargrid_phase.h"]
    assert build.POLAR_HEADERS == ["radargrid_velocity.h"] and build.SHEAR_HEADERS == ["radargrid_shear.h"]
    assert build.HYDRO_HEADERS == ["radargrid_hydro.h"]
    files = build.sources_and_headers()
    assert HEADER in files and os.path.join(build.CSRC, "rg_hydro.hip") in files
    assert files.index(HEADER) > files.index(os.path.join(build.INCLUDE, "radargrid_shear.h"))
    assert set(_native.SHEAR_SIGNATURES) == {"rg_polar_median_f32", "rg_velocity_llsd_f32"}


def test_exports():
    names = ["texture_device", "texture", "MembershipTable", "classify_device", "beam_temperature", "classify_hydrometeors_device",
             "classify_hydrometeors", "class_mask_device", "HYDROMETEOR_TABLE_S_BAND", "HYDROMETEOR_CLASSES", "HYDROMETEOR_VARIABLES",
             "Texture", "FuzzyClasses", "HydrometeorClasses"]
    for name in names:
        assert name in rg.__all__ and getattr(rg, name) is getattr(hydrometeor, name), name
    assert rg.Texture._fields == ("sd", "mean", "count") and rg.FuzzyClasses._fields == ("classes", "score", "second")
    assert rg.HydrometeorClasses._fields == ("classes", "score", "second", "sd_dbz", "sd_phidp")
    assert (hydrometeor.MAX_HALF_GATES, hydrometeor.MAX_VARS, hydrometeor.MAX_CLASSES, hydrometeor.MAX_BINS, hydrometeor.MAX_CELLS) == (63, 8, 16, 32, 1024)


# ---- refusals of the C ABI: each returns before any HIP call ---------------------------------------------------------------------
def texture_args(**kw):
    a = dict(x=P, mask=2 * P, R=40, G=100, half_gates=2, min_valid=3, centre=0, sd=3 * P, mean=4 * P, count=5 * P)
    a.update(kw)
    return (a["x"], a["mask"], a["R"], a["G"], a["half_gates"], a["min_valid"], a["centre"], a["sd"], a["mean"], a["count"], None)


def classify_args(**kw):
    a = dict(vars=(P, 2 * P, 3 * P), kinds=(0, 0, 1), V=3, per_sweep=4, required=1, rps=10, mask=4 * P, R=40, G=100, cond=1, edges=(1.0, 2.0),
             B=3, cells=5 * P, C=2, weights=(1.0, 0.5, 0.0, 0.25, 0.0, 0.0), min_score=0.0, cls=6 * P, score=7 * P, second=8 * P)
    a.update(kw)
    array = lambda ctype, values: None if values is None else (ctype * max(len(values), 1))(*values)     # noqa: E731
    return (array(ctypes.c_void_p, a["vars"]), array(ctypes.c_int32, a["kinds"]), a["V"], a["per_sweep"], a["required"], a["rps"],
            a["mask"], a["R"], a["G"], a["cond"], array(ctypes.c_double, a["edges"]), a["B"], a["cells"], a["C"],
            array(ctypes.c_double, a["weights"]), a["min_score"], a["cls"], a["score"], a["second"], None)


SIZES = [(dict(R=0), "R must be at least 1, got 0"), (dict(G=-1), "G must lie in 0 .. 32768, got -1"),
         (dict(G=32769), "G must lie in 0 .. 32768, got 32769"), (dict(R=65536, G=32768, rps=1), "65536 rays of 32768 gates are 2^31 gates or more")]
N = 40 * 100

REFUSALS = {
    "rg_polar_texture_f32": (texture_args, SIZES + [
        (dict(x=None), "null pointer"), (dict(sd=None, mean=None), "neither sd nor mean is asked for"),
        (dict(half_gates=0), "half_gates must lie in 1 .. 63, got 0"), (dict(half_gates=64), "half_gates must lie in 1 .. 63, got 64"),
        (dict(min_valid=0), "min_valid must lie in 1 .. 127, got 0"), (dict(min_valid=128), "min_valid must lie in 1 .. 127, got 128"),
        (dict(sd=P), "sd overlaps x"), (dict(sd=P + 4 * N - 4), "sd overlaps x"), (dict(mean=P - 4 * N + 4), "mean overlaps x"),
        (dict(count=2 * P + N - 1), "count overlaps mask"), (dict(sd=4 * P + 4), "sd overlaps mean"),
        (dict(mean=5 * P + 2 * N - 4), "mean overlaps count"), (dict(sd=None, count=4 * P), "mean overlaps count")]),
    "rg_fuzzy_classify_f32": (classify_args, SIZES + [
        (dict(vars=None), "null pointer"), (dict(kinds=None), "null pointer"), (dict(weights=None), "null pointer"),
        (dict(cells=None), "null pointer"), (dict(cls=None), "null pointer"),
        (dict(V=0), "V must lie in 1 .. 8, got 0"), (dict(V=9), "V must lie in 1 .. 8, got 9"),
        (dict(C=0), "C must lie in 1 .. 16, got 0"), (dict(C=17), "C must lie in 1 .. 16, got 17"),
        (dict(B=0), "B must lie in 1 .. 32, got 0"), (dict(B=33), "B must lie in 1 .. 32, got 33"),
        (dict(B=32, C=16, weights=(1.0,) * 48, edges=tuple(range(31))), "32 x 16 x 3 cells are more than 1024"),
        (dict(vars=(P, None, 3 * P)), "variable 1 is a null pointer"),
        (dict(kinds=(0, 2, 1)), "the kind of variable 1 must be 0 or 1, got 2"), (dict(kinds=(1, 1, 1)), "no variable is additive"),
        (dict(per_sweep=8), "per_sweep_bits and required_bits must lie in 0 .. 7, got 8 and 1"),
        (dict(required=-1), "per_sweep_bits and required_bits must lie in 0 .. 7, got 4 and -1"),
        (dict(rps=0), "rays_per_sweep must be at least 1 and divide R = 40, got 0"),
        (dict(rps=3), "rays_per_sweep must be at least 1 and divide R = 40, got 3"),
        (dict(cond=3), "cond_var must lie in -1 .. 2, got 3"), (dict(cond=-2), "cond_var must lie in -1 .. 2, got -2"),
        (dict(cond=-1), "3 bins without a condition variable"), (dict(edges=None), "3 bins without edges"),
        (dict(edges=(1.0, INF)), "edge 1 is not finite"), (dict(edges=(NAN, 1.0)), "edge 0 is not finite"),
        (dict(edges=(2.0, 1.0)), "the edges descend at edge 1"),
        (dict(weights=(1.0, 0.5, 0.0, -0.25, 0.0, 0.0)), "weight 0 of class 1 must be finite and not negative, got -0.25"),
        (dict(weights=(1.0, 0.5, INF, 0.25, 0.0, 0.0)), "weight 2 of class 0 must be finite and not negative, got inf"),
        (dict(min_score=-0.5), "min_score must be finite and not negative, got -0.5"), (dict(min_score=NAN), "min_score must be finite and not negative, got nan"),
        (dict(cls=P), "cls overlaps variable 0"), (dict(score=2 * P + 4 * N - 4), "score overlaps variable 1"),
        (dict(second=3 * P + 399), "second overlaps variable 2"), (dict(cls=4 * P + N - 1), "cls overlaps mask"),
        (dict(score=5 * P + 3 * 2 * 3 * 48 - 4), "score overlaps cells"), (dict(cls=7 * P + 4 * N - 1), "cls overlaps score"),
        (dict(cls=8 * P - N + 1), "cls overlaps second"), (dict(score=8 * P), "score overlaps second")]),
}
CASES = [(name, kw, message) for name, (_, cases) in REFUSALS.items() for kw, message in cases]


@pytest.mark.parametrize("name,kw,message", CASES)
def test_refusals_name_the_function_and_the_reason(name, kw, message):
    lib = rg.load_library(require_device=False)
    assert getattr(lib, name)(*REFUSALS[name][0](**kw)) == _native.RG_EINVAL
    assert lib.rg_last_error().decode() == f"{name}: {message}"


def test_alignment_what_does_not_overlap_and_nothing_to_do():
    lib = rg.load_library(require_device=False)
    assert lib.rg_fuzzy_classify_f32(*classify_args(cells=5 * P + 4)) == _native.RG_EALIGN
    assert lib.rg_last_error().decode() == "rg_fuzzy_classify_f32: cells must be 8-byte aligned"
    # a per-sweep variable is a table of R / rays_per_sweep rows: what lies behind it is free
    assert lib.rg_fuzzy_classify_f32(*classify_args(G=0, second=3 * P + 400)) == _native.RG_OK
    # G == 0 returns RG_OK before any launch, whatever coincides: every array is empty
    assert lib.rg_polar_texture_f32(*texture_args(G=0, sd=P, mean=P, count=P)) == _native.RG_OK
    assert lib.rg_polar_texture_f32(*texture_args(G=0, mask=None, mean=None, count=None)) == _native.RG_OK
    assert lib.rg_fuzzy_classify_f32(*classify_args(G=0, score=None, second=None, mask=None)) == _native.RG_OK
    assert lib.rg_fuzzy_classify_f32(*classify_args(G=0, B=1, cond=-1, edges=None, V=1, C=1, per_sweep=0, kinds=(0,), vars=(P,),
                                                    weights=(0.0,))) == _native.RG_OK


# ---- refusals of the wrappers: ValueError before the library is loaded -------------------------------------------------------------
def _small_table(**kw):
    args = dict(classes=("a", "b"), variables=("x", "y"), vertices=np.array([[[0, 1, 2, 3], [0, 0, 5, 5]], [[2, 3, 4, 6], [-INF, -INF, 1, 2]]], float),
                weights=[[1.0, 0.5], [0.25, 0.0]])
    args.update(kw)
    classes, variables, vertices, weights = (args.pop(k) for k in ("classes", "variables", "vertices", "weights"))
    return rg.MembershipTable(classes, variables, vertices, weights, **args)


def test_wrapper_refusals():
    f = np.zeros((6, 20), np.float32)
    table = _small_table()
    huge = np.broadcast_to(np.float32(0), (70000, 32768))
    for call, match in [
            (lambda: rg.texture_device(f.astype(np.float64), half_gates=2), "float32"),
            (lambda: rg.texture_device(f[0], half_gates=2), r"\[n_rays, n_gates\]"), (lambda: rg.texture_device([[1.0]], half_gates=2), "tensor or an ndarray"),
            (lambda: rg.texture_device(np.zeros((0, 4), np.float32), half_gates=2), "at least one ray"),
            (lambda: rg.texture_device(np.zeros((1, 32769), np.float32), half_gates=2), "at most 32768 gates"),
            (lambda: rg.texture_device(huge, half_gates=2), "2\\^31"),
            (lambda: rg.texture_device(f, half_gates=0), "half_gates"), (lambda: rg.texture_device(f, half_gates=64), "half_gates"),
            (lambda: rg.texture_device(f, half_gates=2.0), "half_gates"), (lambda: rg.texture_device(f, half_gates=True), "half_gates"),
            (lambda: rg.texture_device(f, half_gates=2, min_valid=0), "min_valid"), (lambda: rg.texture_device(f, half_gates=2, min_valid=128), "min_valid"),
            (lambda: rg.texture_device(f, half_gates=2, mask=np.zeros((6, 19), np.uint8)), "mask"),
            (lambda: rg.texture(f.astype(np.float16), half_gates=2), "float32"),
            (lambda: rg.classify_device([f, f], None), "MembershipTable"),
            (lambda: rg.classify_device([f], table), "one entry per variable"), (lambda: rg.classify_device(dict(x=f, z=f), table), "does not have"),
            (lambda: rg.classify_device([None, None], table), "at least one"),
            (lambda: rg.classify_device([f, f.astype(np.float64)], table), "float32"), (lambda: rg.classify_device([f, f[:, :5]], table), "variable 'y'"),
            (lambda: rg.classify_device([f, f], table, per_sweep=("z",)), "per_sweep"),
            (lambda: rg.classify_device([f, f[:3]], table, per_sweep=("y",), rays_per_sweep=4), "rays_per_sweep"),
            (lambda: rg.classify_device([f, f[:3]], table, per_sweep=("y",), rays_per_sweep=3), "per sweep"),
            (lambda: rg.classify_device([f, f[:4]], table, per_sweep=("y",)), "rays_per_sweep"),
            (lambda: rg.classify_device([f, f], table, rays_per_sweep=0), "rays_per_sweep"),
            (lambda: rg.classify_device([f, f], table, mask=np.zeros((6, 19), np.uint8)), "mask"),
            (lambda: rg.classify_device([f, f], table, min_score=-1.0), "min_score"), (lambda: rg.classify_device([f, f], table, min_score=NAN), "min_score"),
            (lambda: rg.classify_device([None, f], _small_table(required=("x",))), "required"),
            (lambda: rg.classify_device([f, None], _small_table(condition="y", edges=(1.0,), vertices=np.zeros((2, 2, 2, 4)))), "condition"),
            (lambda: rg.classify_hydrometeors_device(f, f, f, f, table=table), "variables"),
            (lambda: rg.classify_hydrometeors_device(f, None, f, f), "required"),
            (lambda: rg.classify_hydrometeors_device(f[0], f, f, f), r"\[n_rays, n_gates\]"),
            (lambda: rg.classify_hydrometeors_device(f, f[:, :4], f, f), "variable 'ZDR'"),
            (lambda: rg.classify_hydrometeors_device(f, f, f, f, phidp=f[:3]), "phidp"),
            (lambda: rg.classify_hydrometeors_device(f, f, f, f, temperature=np.zeros((4, 20), np.float32)), "rays_per_sweep"),
            (lambda: rg.classify_hydrometeors_device(f, f, f, f, temperature=np.zeros((3, 20), np.float64)), "per sweep"),
            (lambda: rg.classify_hydrometeors_device(f, f, f, f, texture_half_gates=(2,)), "texture_half_gates"),
            (lambda: rg.classify_hydrometeors_device(f, f, f, f, texture_half_gates=(0, 4)), "half_gates"),
            (lambda: rg.classify_hydrometeors_device(f, f, f, f, texture_min_valid=(3,)), "texture_min_valid"),
            (lambda: rg.classify_hydrometeors_device(f, f, f, f, min_score=INF), "min_score"),
            (lambda: rg.classify_hydrometeors(f, f, f, f.astype(np.float64)), "float32"),
            (lambda: rg.class_mask_device(np.zeros((2, 2), np.uint8), table, ("c",)), "no class"),
            (lambda: rg.class_mask_device(np.zeros((2, 2), np.uint8), table, "a"), "sequence"),
            (lambda: rg.class_mask_device(np.zeros((2, 2), np.float32), table, ("a",)), "uint8"),
            (lambda: rg.class_mask_device(np.zeros((2, 2), np.uint8), None, ("a",)), "MembershipTable")]:
        with pytest.raises(ValueError, match=match):
            call()
    assert hydrometeor._check_texture(4, None) == (4, 5) and hydrometeor._check_texture(63, 127) == (63, 127)


def test_membership_table_refusals():
    v = np.array([[[0, 1, 2, 3], [0, 0, 5, 5]], [[2, 3, 4, 6], [-INF, -INF, 1, 2]]], float)
    for kw, match in [(dict(classes=()), "classes"), (dict(classes=("a", "a")), "classes"), (dict(classes=tuple("abcdefghijklmnopq")), "classes"),
                      (dict(variables=("x", 1)), "variables"), (dict(kinds=("additive",)), "kinds"), (dict(kinds=("additive", "other")), "kinds"),
                      (dict(kinds=("multiplicative", "multiplicative")), "additive"), (dict(required=("z",)), "required"),
                      (dict(condition="z"), "condition"), (dict(edges=(1.0,)), "without a condition"),
                      (dict(condition="x", edges=(2.0, 1.0), vertices=np.zeros((3, 2, 2, 4))), "ascend"),
                      (dict(condition="x", edges=(NAN,)), "edges"), (dict(condition="x", edges=tuple(range(32))), "31 edges"),
                      (dict(condition="x", edges="ab"), "edges"),
                      (dict(vertices=v[:1]), r"vertices must be \[1\]\[2\]\[2\]\[4\]"),
                      (dict(vertices=np.where(v == 5, NAN, v)), "NaN"), (dict(vertices=v[..., ::-1]), "ascend"),
                      (dict(vertices=np.where(v == 6, 1e39, v)), "beyond float32"),
                      (dict(vertices=np.where(v == 6, INF, v)), "flank"),           # x4 = inf alone: a flank without a slope
                      (dict(weights=[[1.0, 0.5]]), "weights"), (dict(weights=[[1.0, -0.5], [0, 0]]), "weights"), (dict(weights=[[1.0, INF], [0, 0]]), "weights")]:
        with pytest.raises(ValueError, match=match):
            _small_table(**kw)
    with pytest.raises(ValueError, match="more than 1024 cells"):
        rg.MembershipTable(tuple(f"c{k}" for k in range(16)), tuple(f"v{k}" for k in range(8)), np.zeros((9, 16, 8, 4)), np.ones((16, 8)),
                           condition="v0", edges=tuple(range(8)))
    with pytest.raises(ValueError, match="flank"):
        _small_table(vertices=np.array([[[-INF, 1, 2, 3], [0, 0, 5, 5]], [[2, 3, 4, 6], [0, 0, 1, 2]]], float))


# ---- MembershipTable and beam_temperature against hand-computed values -------------------------------------------------------------
def test_membership_table_compiles_the_cells_worked_out_by_hand():
    t = _small_table(kinds=("additive", "multiplicative"), required=("y",))
    assert (t.n_bins, t.n_classes, t.n_vars, t.cond_var, t.required_bits, t.kinds, t.edges) == (1, 2, 2, -1, 2, (0, 1), ())
    assert t.cells.shape == (1, 2, 2, 6) and t.cells.dtype == np.float64 and not t.cells.flags.writeable
    assert t.cells[0, 0, 0].tolist() == [0.0, 1.0, 2.0, 3.0, 1.0, 1.0]
    assert t.cells[0, 0, 1].tolist() == [0.0, 0.0, 5.0, 5.0, 0.0, 0.0]                  # two steps: no slope
    assert t.cells[0, 1, 0].tolist() == [2.0, 3.0, 4.0, 6.0, 1.0, 0.5]
    assert t.cells[0, 1, 1].tolist() == [-INF, -INF, 1.0, 2.0, 0.0, 1.0]                # an open shoulder: no slope
    assert t.class_value("b") == 2 and t.weights.tolist() == [[1.0, 0.5], [0.25, 0.0]]
    # vertices are rounded to float32 FIRST, the reciprocals come from the rounded values
    t = _small_table(vertices=np.array([[[0.1, 0.3, 0.7, 1.0], [0, 0, 5, 5]], [[2, 3, 4, 6], [0, 0, 1, 2]]]), condition=None)
    a, b, c = (float(np.float32(x)) for x in (0.1, 0.3, 0.7))
    assert t.cells[0, 0, 0].tolist() == [a, b, c, 1.0, 1.0 / (b - a), 1.0 / (1.0 - c)] and a != 0.1
    assert np.array_equal(t.cells, ho.compile_cells(t.vertices))
    # [C][V][4] is taken for every bin
    t = _small_table(condition="x", edges=(1.5, 2.5))
    assert t.cells.shape == (3, 2, 2, 6) and np.array_equal(t.cells[0], t.cells[2]) and t.cond_var == 0 and t.n_bins == 3


def test_beam_temperature_against_hand_computed_values():
    ke_re = (4.0 / 3.0) * rg.EARTH_RADIUS
    ranges = np.array([0.0, 10000.0, 100000.0])
    sounding_h, sounding_t = np.array([0.0, 2000.0, 10000.0]), np.array([20.0, 10.0, -50.0])
    got = rg.beam_temperature([0.0, 10.0], ranges, sounding_h, sounding_t, radar_altitude=500.0)
    assert got.shape == (2, 3) and got.dtype == np.float32
    want = np.empty((2, 3))
    for s, el in enumerate((0.0, 10.0)):
        for k, ground in enumerate(ranges):
            slant = ground / math.cos(math.radians(el))
            h = math.sqrt(slant * slant + ke_re * ke_re + 2.0 * slant * ke_re * math.sin(math.radians(el))) - ke_re + 500.0
            if h <= 2000.0:
                want[s, k] = 20.0 - 10.0 * h / 2000.0
            elif h <= 10000.0:
                want[s, k] = 10.0 - 60.0 * (h - 2000.0) / 8000.0
            else:
                want[s, k] = -50.0                                           # constant beyond the sounding
    assert np.allclose(got, want, rtol=0, atol=1e-4)
    assert got[0, 0] == np.float32(17.5) and got[1, 0] == np.float32(17.5) and got[1, 2] == np.float32(-50.0)
    h = rg.compute_beam_height(ranges, 10.0, 500.0)
    assert np.array_equal(got[1], np.interp(h, sounding_h, sounding_t).astype(np.float32))
    assert rg.beam_temperature(1.0, ranges, [0.0], [5.0]).tolist() == [[5.0, 5.0, 5.0]]
    for args, match in [(([[0.5]], ranges, sounding_h, sounding_t), "elevations_deg"), (([NAN], ranges, sounding_h, sounding_t), "elevations_deg"),
                        (([0.5], ranges[None], sounding_h, sounding_t), "ranges_m"), (([0.5], ranges, sounding_h[::-1], sounding_t), "ascend"),
                        (([0.5], ranges, sounding_h, sounding_t[:2]), "one length"), (([0.5], ranges, [], []), "not empty")]:
        with pytest.raises(ValueError, match=match):
            rg.beam_temperature(*args)


# ---- the preset ------------------------------------------------------------------------------------------------------------------
def _preset_class(z, zdr, kdp, rhohv, sd_z, sd_p, t):
    table = rg.HYDROMETEOR_TABLE_S_BAND
    fields = [np.full((1, 1), np.float32(v)) for v in (z, zdr, kdp, rhohv, sd_z, sd_p, t)]
    got = ho.classify(fields, 1 << 6, 1, None, ho.spec_of(table), 0.0)
    naive = ho.classify_naive(fields, 1 << 6, 1, None, ho.spec_of(table), 0.0)
    assert got.cls[0, 0] == naive.cls[0, 0] and got.second[0, 0] == naive.second[0, 0]
    return "unclassified" if got.cls[0, 0] == 0 else table.class_names[got.cls[0, 0] - 1]


def test_the_preset_is_what_it_says_and_archetypes_land_in_their_class():
    t = rg.HYDROMETEOR_TABLE_S_BAND
    assert t.class_names == rg.HYDROMETEOR_CLASSES == ("ground clutter", "biological", "dry snow", "wet snow", "crystals", "graupel",
                                                        "big drops", "rain", "heavy rain", "rain and hail")
    assert t.variable_names == rg.HYDROMETEOR_VARIABLES == ("Z", "ZDR", "KDP", "RHOHV", "SD(Z)", "SD(PHIDP)", "T")
    assert t.condition == "Z" and t.edges == tuple(float(e) for e in range(5, 70, 5)) and t.n_bins * 10 * 7 == 980 <= 1024
    assert t.kinds == (1, 0, 0, 0, 0, 0, 1) and set(t.required) == {"Z", "ZDR", "RHOHV"}
    assert "PRESET" in hydrometeor.__doc__ + (hydrometeor.HYDROMETEOR_TABLE_S_BAND.__class__.__doc__ or "") or "PRESET" in open(hydrometeor.__file__).read()
    assert _preset_class(35.0, 1.0, 0.3, 0.99, 1.0, 5.0, 15.0) == "rain"                    # warm rain
    assert _preset_class(18.0, 0.15, 0.02, 0.995, 0.8, 4.0, -12.0) == "dry snow"            # a cold, low-Z, low-ZDR aggregate
    assert _preset_class(62.0, 0.1, 2.0, 0.97, 1.5, 8.0, 8.0) == "rain and hail"            # a 62 dBZ, near-zero-ZDR core above 0 C
    assert _preset_class(30.0, -1.0, 0.0, 0.75, 6.0, 45.0, 12.0) == "ground clutter"        # a noisy low-RHOHV echo
    assert _preset_class(35.0, 1.0, 0.3, 0.99, 1.0, 5.0, NAN) == "rain"                     # a missing temperature still classifies
    assert _preset_class(35.0, 1.0, NAN, 0.99, NAN, NAN, NAN) == "rain"                     # ... and so do missing optional variables
    assert _preset_class(35.0, NAN, 0.3, 0.99, 1.0, 5.0, 15.0) == "unclassified"            # ZDR is required
    assert _preset_class(NAN, 1.0, 0.3, 0.99, 1.0, 5.0, 15.0) == "unclassified"             # Z is the condition variable


# ---- the two restatements check each other ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["shape_3x65_L2", "shape_1x2_L1", "shape_1x127_L63", "shape_3x128_L63", "holes_mask", "empty_rays", "limits",
                                  "constant", "min_valid_at_n", "min_valid_above_n"])
def test_vectorised_texture_equals_the_naive_one(name):
    s = hs.texture_scenes()[name]
    fast, slow = hs.texture_reference(name), ho.texture_naive(*hs.texture_args(s))
    assert np.array_equal(fast.count, slow.count)
    assert np.array_equal(ho.bits(fast.sd), ho.bits(slow.sd)) and np.array_equal(ho.bits(fast.mean), ho.bits(slow.mean))


@pytest.mark.parametrize("name", sorted(set(hs.classifier_scenes()) - {"strides"}))
def test_vectorised_classifier_equals_the_naive_one_on_tiny_cuts_of_the_scenes(name):
    s = hs.tiny(hs.classifier_scenes()[name], 3, 120)
    fast, slow = ho.classify(*hs.classifier_args(s)), ho.classify_naive(*hs.classifier_args(s))
    assert np.array_equal(fast.cls, slow.cls) and np.array_equal(fast.second, slow.second)
    assert np.array_equal(ho.bits(fast.score), ho.bits(slow.score))
    assert np.array_equal(fast.best.view(np.uint64), slow.best.view(np.uint64))
    assert (fast.cls != 0).any()
