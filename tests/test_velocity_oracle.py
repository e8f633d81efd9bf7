"""CPU-side checks of the velocity dealiasing (no GPU needed): the fourth header against ``_native.VELOCITY_SIGNATURES``, the build
lists, the exports, the refusals of the wrappers and of the entry points (all of which return before any HIP call), and the host
merge (a heap and a union-find) against the restatement's naive scan."""
import ctypes
import os
import re

import numpy as np
import pytest

import radar_processor_amd as rg
from radar_processor_amd import _native, velocity

import velocity_oracle as vo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "radargrid_velocity.h")
NAMES = {"rg_velocity_split_f32", "rg_velocity_regions_i32", "rg_region_edges_workspace_bytes", "rg_region_edges_f32",
         "rg_velocity_apply_folds_f32"}
P = 1 << 20                                  # an aligned address that is never dereferenced
NAN, INF = float("nan"), float("inf")


# ---- the fourth header -----------------------------------------------------------------------------------------------------------
def _declared():
    """name -> (return type, [(C type, argument name)]) of every function the header declares."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"^(int|int64_t)\s+(rg_\w+)\s*\(([^;]*)\);", text, flags=re.M):
        out[name] = (ret, [tuple(a.strip().rsplit(" ", 1)) for a in args.replace("\n", " ").split(",")])
    return out


def _ctype(ctype, name):
    if name.endswith("_host"):
        return {"const double*": ctypes.POINTER(ctypes.c_double)}[ctype]
    if ctype.endswith("*") or ctype == "rg_stream_t":
        return ctypes.c_void_p
    return {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}[ctype]


def test_header_and_table_mirror_each_other_one_to_one():
    declared = _declared()
    assert set(declared) == set(_native.VELOCITY_SIGNATURES) == NAMES
    for table in (_native.SIGNATURES, _native.ENSEMBLE_SIGNATURES, _native.PHASE_SIGNATURES):
        assert not NAMES & set(table)
    lib = rg.load_library(require_device=False)
    raw = ctypes.CDLL(_native.LIB_PATH)
    for name, (ret, args) in declared.items():
        restype, argtypes = _native.VELOCITY_SIGNATURES[name]
        assert restype is {"int": ctypes.c_int32, "int64_t": ctypes.c_int64}[ret], name
        assert argtypes == [_ctype(*a) for a in args], name
        if name != "rg_region_edges_workspace_bytes":
            assert args[-1] == ("rg_stream_t", "stream"), f"{name}: the stream comes last"
        assert hasattr(raw, name), f"{name} declared in the header but not exported"
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    header = open(HEADER).read()
    assert '#include "radargrid_hip.h"' in header
    for macro in ("RG_VELOCITY_MAX_ABS", "RG_VELOCITY_MAX_NYQUIST", "RG_VELOCITY_MIN_BANDS", "RG_VELOCITY_MAX_BANDS",
                  "RG_VELOCITY_SWEEPS_PER_LAUNCH"):
        assert re.search(r"#define %s %d\b" % (macro, getattr(_native, macro)), header), macro
    assert lib.rg_version() == _native.ABI_VERSION == 104


def test_the_new_unit_and_header_are_part_of_the_build():
    from radar_processor_amd import build
    assert ("rg_velocity.hip", []) in build.SOURCES and build.SOURCES[-1] == ("rg_warp.hip", [])
    assert build.PUBLIC_HEADERS == ["radargrid_hip.h", "radargrid_ensemble.h", "radargrid_phase.h"]
    assert build.POLAR_HEADERS == ["radargrid_velocity.h"]
    files = build.sources_and_headers()
    assert HEADER in files and os.path.join(build.CSRC, "rg_velocity.hip") in files
    assert files.index(HEADER) > files.index(os.path.join(build.INCLUDE, "radargrid_phase.h"))


def test_exports():
    names = ["split_velocity_device", "velocity_regions_device", "region_edges_device", "merge_regions", "apply_folds_device",
             "dealias_velocity_device", "dealias_velocity", "VelocityRegions", "RegionEdges", "DealiasedVelocity"]
    for name in names:
        assert name in rg.__all__ and getattr(rg, name) is getattr(velocity, name), name
    assert rg.VelocityRegions._fields == ("regions", "n_regions", "sizes", "cell_ptr")
    assert rg.RegionEdges._fields == ("pairs", "count", "sum", "totals")
    assert rg.DealiasedVelocity._fields == ("velocity", "folds", "regions", "n_regions", "n_edges")
    assert velocity.interval_of(10.0) == 65536 * 20 == vo.interval(10.0)
    assert velocity.default_max_edges(5) == 64 and velocity.default_max_edges(1000) == 3000


# ---- refusals of the wrappers: ValueError before the library is loaded -------------------------------------------------------------
def test_wrapper_refusals():
    v = np.zeros((2, 3, 20), np.float32)
    r = np.zeros((2, 3, 20), np.int32)
    lut = np.zeros(4, np.int32)
    for call, match in [
            (lambda: rg.split_velocity_device(v.astype(np.float64), 10.0), "float32"),
            (lambda: rg.split_velocity_device(v[0, 0], 10.0), r"\[n_sweeps, n_rays, n_gates\]"),
            (lambda: rg.split_velocity_device(np.zeros((0, 3, 4), np.float32), 10.0), "at least one sweep"),
            (lambda: rg.split_velocity_device(np.zeros((1, 0, 4), np.float32), 10.0), "one ray"),
            (lambda: rg.split_velocity_device([[1.0]], 10.0), "tensor or an ndarray"),
            (lambda: rg.split_velocity_device(v, 10.0, n_bands=1), "n_bands"), (lambda: rg.split_velocity_device(v, 10.0, n_bands=9), "n_bands"),
            (lambda: rg.split_velocity_device(v, 10.0, n_bands=3.0), "n_bands"), (lambda: rg.split_velocity_device(v, 10.0, n_bands=True), "n_bands"),
            (lambda: rg.split_velocity_device(v, 0.0), "nyquist"), (lambda: rg.split_velocity_device(v, -3.0), "nyquist"),
            (lambda: rg.split_velocity_device(v, NAN), "nyquist"), (lambda: rg.split_velocity_device(v, INF), "nyquist"),
            (lambda: rg.split_velocity_device(v, 8192.5), "nyquist"), (lambda: rg.split_velocity_device(v, 1e-9), "nyquist"),
            (lambda: rg.split_velocity_device(v, (10.0, 9.0, 8.0)), "one per sweep"),
            (lambda: rg.split_velocity_device(v, "fast"), "nyquist"),
            (lambda: rg.split_velocity_device(v, 10.0, mask=np.zeros((2, 3, 19), np.uint8)), "mask"),
            (lambda: rg.split_velocity_device(np.broadcast_to(np.float32(0), (2, 40000, 10000)), 10.0), "2\\^31"),
            (lambda: rg.velocity_regions_device(v, (10.0,)), "one per sweep"),
            (lambda: rg.velocity_regions_device(v[0], (10.0, 10.0)), "one per sweep"),
            (lambda: rg.velocity_regions_device(v, 10.0, n_bands=0), "n_bands"),
            (lambda: rg.region_edges_device(v, r[0], wrap_rows=True), "differ"),
            (lambda: rg.region_edges_device(v, r.astype(np.int64), wrap_rows=True), "int32"),
            (lambda: rg.region_edges_device(v.astype(np.float64), r, wrap_rows=True), "float32"),
            (lambda: rg.region_edges_device(v, r, wrap_rows=True, max_edges=0), "max_edges"),
            (lambda: rg.region_edges_device(v, r, wrap_rows=True, max_edges=2 ** 30), "max_edges"),
            (lambda: rg.region_edges_device(v, r, wrap_rows=True, max_edges=2.5), "max_edges"),
            (lambda: rg.apply_folds_device(v, r.astype(np.int64), lut, 10.0), "regions must be int32"),
            (lambda: rg.apply_folds_device(v, r[:, :, :5], lut, 10.0), "regions"),
            (lambda: rg.apply_folds_device(v, None, lut, 10.0), "regions is required"),
            (lambda: rg.apply_folds_device(v, r, lut.astype(np.int64), 10.0), "fold_lut"),
            (lambda: rg.apply_folds_device(v, r, lut[None], 10.0), "fold_lut"),
            (lambda: rg.apply_folds_device(v, r, lut, 0.0), "nyquist"),
            (lambda: rg.dealias_velocity_device(v, 10.0, n_bands=12), "n_bands"),
            (lambda: rg.dealias_velocity_device(v, (10.0, NAN)), "nyquist"),
            (lambda: rg.dealias_velocity(v, 10.0, mask=np.zeros((3, 20), np.uint8)), "mask")]:
        with pytest.raises(ValueError, match=match):
            call()
    with pytest.raises(TypeError):
        rg.region_edges_device(v, r)                                          # wrap_rows has no default


def test_merge_regions_refuses_what_is_not_an_edge_table():
    for edges, sizes, intervals, match in [
            ([(1, 2, 3, 0)], [4, 4], [100], "interval_of_region"),
            ([(1, 2, 3, 0)], [4, 4], [100, 0], "at least 1"),
            ([(2, 1, 3, 0)], [4, 4], [100, 100], "lo < hi"),
            ([(1, 3, 3, 0)], [4, 4], [100, 100], "lo < hi"),
            ([(1, 2, 0, 0)], [4, 4], [100, 100], "count >= 1"),
            ([(1, 2, 3, 0), (1, 2, 1, 5)], [4, 4], [100, 100], "twice")]:
        with pytest.raises(ValueError, match=match):
            rg.merge_regions(edges, sizes, intervals)


# ---- refusals of the C ABI: each returns before any HIP call ---------------------------------------------------------------------
def _nyq(values):
    return None if values is None else (ctypes.c_double * max(len(values), 1))(*values)


def split_args(**kw):
    a = dict(vel=P, mask=2 * P, S=2, R=4, G=100, nyquist=[10.0, 8.0], n_bands=3, split=4 * P)
    a.update(kw)
    return a["vel"], a["mask"], a["S"], a["R"], a["G"], _nyq(a["nyquist"]), a["n_bands"], a["split"], None


def regions_args(**kw):
    a = dict(labels=P, cell_ptr=2 * P, S=2, R=4, G=100, n_bands=3, regions=4 * P)
    a.update(kw)
    return a["labels"], a["cell_ptr"], a["S"], a["R"], a["G"], a["n_bands"], a["regions"], None


def edges_args(**kw):
    a = dict(values=P, regions=2 * P, n=2, h=4, w=100, wrap=1, max_edges=100, ids=3 * P, count=4 * P, sum=5 * P, totals=6 * P,
             workspace=7 * P, bytes=1 << 16)
    a.update(kw)
    return (a["values"], a["regions"], a["n"], a["h"], a["w"], a["wrap"], a["max_edges"], a["ids"], a["count"], a["sum"], a["totals"],
            a["workspace"], a["bytes"], None)


def apply_args(**kw):
    a = dict(vel=P, regions=2 * P, lut=3 * P, n_regions=50, S=2, R=4, G=100, nyquist=[10.0, 8.0], out=4 * P, folds=5 * P)
    a.update(kw)
    return (a["vel"], a["regions"], a["lut"], a["n_regions"], a["S"], a["R"], a["G"], _nyq(a["nyquist"]), a["out"], a["folds"], None)


BANDS = [(dict(n_bands=1), "n_bands must lie in 2 .. 8, got 1"), (dict(n_bands=9), "n_bands must lie in 2 .. 8, got 9")]
NYQUIST = [(dict(nyquist=[10.0, 0.0]), "the Nyquist velocity of sweep 1 must be finite with 0 < Vn <= 8192, got 0"),
           (dict(nyquist=[-1.0, 8.0]), "the Nyquist velocity of sweep 0 must be finite with 0 < Vn <= 8192, got -1"),
           (dict(nyquist=[NAN, 8.0]), "the Nyquist velocity of sweep 0 must be finite with 0 < Vn <= 8192, got nan"),
           (dict(nyquist=[10.0, INF]), "the Nyquist velocity of sweep 1 must be finite with 0 < Vn <= 8192, got inf"),
           (dict(nyquist=[8192.5, 8.0]), "the Nyquist velocity of sweep 0 must be finite with 0 < Vn <= 8192, got 8192.5")]


def _sizes(planes):
    return [(dict(S=0), "S and R must be at least 1, got 0 and 4"), (dict(R=0), "S and R must be at least 1, got 2 and 0"),
            (dict(G=-1), "G must not be negative, got -1"),
            (dict(S=2, R=32768, G=32768 // planes), f"2 sweeps x {planes} plane(s) of 32768 x {32768 // planes} are 2^31 gates or more")]


REFUSALS = {
    "rg_velocity_split_f32": (split_args, BANDS + _sizes(3)[:3] + NYQUIST + [
        (dict(S=2, R=32768, G=10923), "2 sweeps x 3 plane(s) of 32768 x 10923 are 2^31 gates or more"),
        (dict(vel=None), "null pointer"), (dict(nyquist=None), "null pointer"), (dict(split=None), "null pointer"),
        (dict(split=P + 4), "split overlaps vel"), (dict(split=2 * P + 799), "split overlaps mask"), (dict(vel=4 * P + 9596), "split overlaps vel")]),
    "rg_velocity_regions_i32": (regions_args, BANDS + _sizes(3)[:3] + [
        (dict(labels=None), "null pointer"), (dict(cell_ptr=None), "null pointer"), (dict(regions=None), "null pointer"),
        (dict(regions=P + 9596), "regions overlaps labels"), (dict(regions=2 * P + 24), "regions overlaps cell_ptr"),
        (dict(regions=2 * P - 3196), "regions overlaps cell_ptr")]),
    "rg_region_edges_f32": (edges_args, [
        (dict(n=0), "n_planes must be at least 1, got 0"), (dict(h=-1), "negative size -1 x 100"), (dict(w=-2), "negative size 4 x -2"),
        (dict(n=2, h=32768, w=32768), "2 planes of 32768 x 32768 are 2^31 pixels or more"),
        (dict(max_edges=0), "max_edges must lie in 1 .. 2^30 - 1, got 0"),
        (dict(max_edges=2 ** 30), "max_edges must lie in 1 .. 2^30 - 1, got 1073741824"),
        (dict(values=None), "null pointer"), (dict(regions=None), "null pointer"), (dict(ids=None), "null pointer"),
        (dict(count=None), "null pointer"), (dict(sum=None), "null pointer"), (dict(totals=None), "null pointer"),
        (dict(workspace=None), "null pointer"),
        (dict(ids=P + 8), "pair_ids overlaps values"), (dict(count=2 * P + 3196), "pair_count overlaps regions"),
        (dict(sum=P - 792), "pair_sum overlaps values"), (dict(totals=2 * P), "totals overlaps regions"),
        (dict(workspace=P + 3192), "workspace overlaps values"), (dict(workspace=2 * P - 5112), "workspace overlaps regions")]),
    "rg_velocity_apply_folds_f32": (apply_args, _sizes(1) + NYQUIST + [
        (dict(vel=None), "null pointer"), (dict(regions=None), "null pointer"), (dict(nyquist=None), "null pointer"),
        (dict(out=None), "null pointer"), (dict(lut=None), "null pointer"), (dict(n_regions=-1), "negative n_regions -1"),
        (dict(out=P + 4), "out overlaps vel"), (dict(out=2 * P), "out overlaps regions"), (dict(out=3 * P + 196), "out overlaps fold_lut"),
        (dict(folds=P), "folds overlaps vel"), (dict(folds=2 * P + 3196), "folds overlaps regions"), (dict(folds=3 * P), "folds overlaps fold_lut"),
        (dict(folds=4 * P + 3196), "out overlaps folds"), (dict(out=P, folds=P), "out overlaps folds")]),
}
CASES = [(name, kw, message) for name, (_, cases) in REFUSALS.items() for kw, message in cases]


@pytest.mark.parametrize("name,kw,message", CASES)
def test_refusals_name_the_function_and_the_reason(name, kw, message):
    lib = rg.load_library(require_device=False)
    assert getattr(lib, name)(*REFUSALS[name][0](**kw)) == _native.RG_EINVAL
    assert lib.rg_last_error().decode() == f"{name}: {message}"


def test_alignment_workspace_and_the_workspace_size():
    lib = rg.load_library(require_device=False)
    for max_edges, capacity in [(1, 64), (32, 64), (33, 128), (100, 256), (3000, 8192), (2 ** 30 - 1, 2 ** 31)]:
        assert lib.rg_region_edges_workspace_bytes(max_edges) == 20 * capacity
    for bad in (0, -1, 2 ** 30):
        assert lib.rg_region_edges_workspace_bytes(bad) == _native.RG_EINVAL
        assert lib.rg_last_error().decode().startswith("rg_region_edges_workspace_bytes: max_edges must lie in 1 .. 2^30 - 1")
    assert lib.rg_region_edges_f32(*edges_args(sum=5 * P + 4)) == _native.RG_EALIGN
    assert lib.rg_region_edges_f32(*edges_args(workspace=7 * P + 4)) == _native.RG_EALIGN
    assert lib.rg_region_edges_f32(*edges_args(values=P + 2)) == _native.RG_EALIGN
    assert lib.rg_last_error().decode().startswith("rg_region_edges_f32: ")
    assert lib.rg_region_edges_f32(*edges_args(bytes=20 * 256 - 1)) == _native.RG_EWORKSPACE
    assert lib.rg_last_error().decode() == "rg_region_edges_f32: workspace of 5119 bytes, 5120 needed"


def test_nothing_to_do_and_the_allowed_in_place_use_are_ok_without_a_launch():
    """G == 0 returns RG_OK before any launch, whatever coincides: every array is empty."""
    lib = rg.load_library(require_device=False)
    assert lib.rg_velocity_split_f32(*split_args(G=0, split=P)) == _native.RG_OK
    assert lib.rg_velocity_split_f32(*split_args(G=0, mask=None)) == _native.RG_OK
    assert lib.rg_velocity_regions_i32(*regions_args(G=0)) == _native.RG_OK
    assert lib.rg_velocity_apply_folds_f32(*apply_args(G=0, out=P, folds=None, lut=None, n_regions=0)) == _native.RG_OK


# ---- the host merge against the naive scan -----------------------------------------------------------------------------------------
def _check(edges, sizes, intervals):
    got = rg.merge_regions(edges, sizes, intervals)
    want = vo.merge(edges, sizes, intervals)
    assert got.dtype == np.int64 and np.array_equal(got, want), (edges, sizes, intervals, got, want)
    return got


def random_graph(rng, n, p_edge, groups=1, big=False):
    """A random graph on n regions in `groups` groups of one interval each (edges stay inside a group), with many ties in count
    and in size."""
    group = np.sort(rng.integers(0, groups, n))
    interval = [(65536 * 20, 65536 * 13 + 77, 999_983)[g % 3] for g in group]
    sizes = rng.integers(1, 4, n) if not big else rng.integers(1, 2000, n)
    edges = []
    for lo in range(1, n + 1):
        for hi in range(lo + 1, n + 1):
            if group[lo - 1] == group[hi - 1] and rng.random() < p_edge:
                c = int(rng.integers(1, 4)) if not big else int(rng.integers(1, 300))
                i = interval[lo - 1]
                s = int(rng.integers(-3, 4)) * c * i + int(rng.integers(-i // 2, i // 2 + 1)) * c // 2
                edges.append((lo, hi, c, s))
    return edges, sizes.tolist(), interval


@pytest.mark.parametrize("seed", range(40))
def test_merge_regions_equals_the_naive_scan_on_random_graphs(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 30))
    edges, sizes, interval = random_graph(rng, n, float(rng.choice([0.08, 0.2, 0.5])), groups=int(rng.integers(1, 4)), big=seed % 4 == 3)
    _check(edges, sizes, interval)


def test_merge_ties_in_count_and_in_size():
    i = 1000
    # all counts equal, all sizes equal: the order is by (lo, hi) alone and the base by the smaller name
    edges = [(1, 2, 5, 1 * 5 * i + 7), (2, 3, 5, -2 * 5 * i), (1, 3, 5, 3), (3, 4, 5, 5 * i), (4, 5, 5, -5 * i + 1)]
    got = _check(edges, [3, 3, 3, 3, 3], [i] * 5)
    assert len(set(got.tolist())) > 1
    # the larger set is the base although it has the larger name
    assert _check([(1, 2, 4, 4 * i)], [1, 9], [i, i]).tolist() == [1, 0]
    assert _check([(1, 2, 4, 4 * i)], [9, 1], [i, i]).tolist() == [0, -1]
    # equal sizes: the smaller name is the base; the centring then breaks the tie of gates by |fold| and sign
    assert _check([(1, 2, 4, 4 * i)], [5, 5], [i, i]).tolist() == [0, -1]
    assert _check([(1, 2, 4, -4 * i)], [5, 5], [i, i]).tolist() == [0, 1]
    assert _check([(1, 2, 1, 2 * i), (2, 3, 1, 2 * i)], [2, 2, 2], [i] * 3).tolist() == [0, -2, -4]


def test_merge_an_exact_half_rounds_up():
    i, c = 1000, 6
    w = c * i
    # 2 S == W: n = 1; 2 S == -W: n = 0; one below the half: n = 0 and n = -1
    for s, n in [(w // 2, 1), (-w // 2, 0), (w // 2 - 1, 0), (-w // 2 - 1, -1), (3 * w // 2, 2), (-3 * w // 2, -1)]:
        assert 2 * abs(s) in (w, 3 * w) or 2 * abs(s) in (w - 2, w + 2)
        got = _check([(1, 2, c, s)], [9, 1], [i, i])             # region 2 is M, S is already oriented M - base
        assert got.tolist() == [0, -n], (s, n)
        got = _check([(1, 2, c, -s)], [1, 9], [i, i])            # region 1 is M: S oriented M - base is s again
        assert got.tolist() == [-n, 0], (s, n)


def test_merge_two_sweeps_with_different_intervals_and_disconnected_sets():
    i1, i2 = 65536 * 20, 65536 * 13
    edges = [(1, 2, 10, 10 * i1 + 5), (2, 3, 4, -4 * i1), (4, 5, 10, 10 * i2 - 3), (5, 6, 2, 4 * i2 + 1)]
    sizes = [50, 20, 5, 50, 20, 5, 7, 1]
    got = _check(edges, sizes, [i1] * 3 + [i2] * 3 + [i1, i2])
    assert got.tolist() == [0, -1, 0, 0, -1, -3, 0, 0]
    # with the first sweep's interval on the second sweep's regions the folds would differ: the interval is per region
    other = _check(edges, sizes, [i1] * 3 + [i1] * 3 + [i1, i2])
    assert other.tolist() != got.tolist()
    # no edges at all, and no regions at all
    assert _check([], [3, 4], [i1, i1]).tolist() == [0, 0]
    assert rg.merge_regions([], [], []).shape == (0,)
    assert rg.merge_regions(np.zeros((0, 4), np.int64), np.zeros(0, np.int32), np.zeros(0, np.int64)).shape == (0,)


def test_merge_of_a_chain_moves_later_edges_with_the_merged_set():
    """1 - 2 - 3 - 4 in a row, each step one interval up: the strongest edge merges first and the others are re-oriented."""
    i = 500
    edges = [(1, 2, 3, 3 * i), (2, 3, 9, 9 * i), (3, 4, 5, 5 * i), (1, 4, 1, 3 * i)]
    got = _check(edges, [10, 20, 30, 40], [i] * 4)
    assert got.tolist() == [3, 2, 1, 0]


def test_merge_regions_on_the_scenes_equals_the_restatement():
    import velocity_scenes as vs
    for name in vs.scenes():
        s, ref = vs.scenes()[name], vs.reference(name)
        reg = vo.regions(s.vel, s.nyquist, s.n_bands, s.mask, s.wrap)
        S = vo.as_volume(s.vel).shape[0]
        intervals = velocity.region_intervals(reg.cell_ptr, vo.nyquists(s.nyquist, S).tolist(), s.n_bands)
        assert intervals.tolist() == vo.region_intervals(reg.cell_ptr, s.nyquist, s.n_bands)
        assert np.array_equal(rg.merge_regions(ref.edges, reg.sizes, intervals), ref.lut), name
