"""The mosaic combine rules, CPU side: the NumPy restatement (tests/combine_scenes.py: fold) on hand-made stacks, what the tie
scene and scene16 exercise (counted from the oracle's per-radar float64 means), the new symbols of the C ABI and their
refusals (every call fails validation before a launch), and the ValueErrors of the Python surface, raised without a device."""
import os
import re

import numpy as np
import pytest

import combine_scenes as cs
import radar_processor_amd as rg
from radar_processor_amd import _native, mosaic

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 12                                  # a 16-byte aligned address that is never dereferenced
F = np.float32


# ---- 1. the fold restatement ----------------------------------------------------------------------------------------------------
def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


def test_fold_max_on_hand_made_stacks():
    nan = F(np.nan)
    #                 tie   later larger  NaN first  NaN later  -0 then +0  +0 then -0  nobody  only last  inf
    values = np.array([[1.5, 1.0, nan, 2.0, -0.0, 0.0, 7.0, 7.0, 1.0],
                       [1.5, 3.0, 4.0, nan, 0.0, -0.0, 7.0, 7.0, np.inf],
                       [0.5, 2.0, 3.0, 1.0, 0.0, 0.0, 7.0, 5.0, nan]], dtype=np.float32)
    has = np.ones(values.shape, dtype=bool)
    has[:, 6] = False                        # nobody has a value: the 7.0 there must not be looked at
    has[:2, 7] = False                       # only the last radar has one
    out, who = cs.fold(values, has, "max", fill=-1.0)
    assert who.tolist() == [0, 1, 1, 0, 0, 0, 255, 2, 1]
    np.testing.assert_array_equal(_bits(out), _bits([1.5, 3.0, 4.0, 2.0, -0.0, 0.0, -1.0, 5.0, np.inf]))
    # a NaN is held until a number comes; with NaN only, the first one stays (its bits, payload included)
    payload = np.array([0x7FC00123, 0x7FC00456], dtype=np.int32).view(np.float32)
    out, who = cs.fold(payload[:, None], np.ones((2, 1), dtype=bool), "max")
    assert who.tolist() == [0] and _bits(out).tolist() == [0x7FC00123]
    # a radar without a value never takes over, however large what its grid holds
    out, who = cs.fold(np.array([[1.0], [9.0]], F), np.array([[True], [False]]), "max")
    assert who.tolist() == [0] and out.tolist() == [1.0]
    assert out.dtype == np.float32 and who.dtype == np.uint8


def test_fold_nearest_radar_on_hand_made_stacks():
    values = np.array([[1.0, 1.0, 1.0, 1.0, np.nan], [2.0, 2.0, 2.0, 2.0, 2.0], [3.0, 3.0, 3.0, 3.0, 3.0]], dtype=np.float32)
    #            nearest last  tie 0 = 1   nearest has no value  nobody   a NaN of the nearest radar is its value
    d = np.array([[9.0, 4.0, 1.0, 1.0, 1.0], [5.0, 4.0, 2.0, 1.0, 2.0], [4.0, 6.0, 3.0, 1.0, 3.0]])
    has = np.ones(values.shape, dtype=bool)
    has[0, 2] = False
    has[:, 3] = False
    out, who = cs.fold(values, has, "nearest_radar", d, fill=-1.0)
    assert who.tolist() == [2, 0, 1, 255, 0]
    np.testing.assert_array_equal(_bits(out), _bits([3.0, 1.0, 2.0, -1.0, np.nan]))
    # D differing in the last bit of a float64 decides
    d = np.array([[np.nextafter(1e8, 2e8)], [1e8]])
    assert cs.fold(values[:2, :1], np.ones((2, 1), bool), "nearest_radar", d)[1].tolist() == [1]
    with pytest.raises(ValueError):
        cs.fold(values, has, "mean")


def test_antenna_d2_is_float64_and_unfused():
    x, y, z = F(12345.678), F(-23456.789), F(3456.789)
    want = (float(x) * float(x) + float(y) * float(y)) + float(z) * float(z)
    assert cs.antenna_d2(x, y, z) == want and cs.antenna_d2(x, y, z).dtype == np.float64
    assert cs.antenna_d2(F(-9000.0), y, z) == cs.antenna_d2(F(9000.0), y, z)


# ---- 2. what the scenes exercise ----------------------------------------------------------------------------------------------
def _cases(name, k, section=False):
    scene = cs.scene(name)
    fs, shared = cs.field_set(scene, 3)
    radars = range(scene.n_radars)
    if section:
        xs, ys = cs.path(name)
        stats = [cs.radar_stats(scene, "barnes2", fs, shared, k, r, cs.section_pairs(scene, "barnes2", r, xs, ys, "combine"))
                 for r in radars]
        d = np.stack([cs.section_d(scene, r, xs, ys).ravel() for r in radars])
    else:
        stats = [cs.radar_stats(scene, "barnes2", fs, shared, k, r) for r in radars]
        d = np.stack([cs.lattice_d(scene, r).ravel() for r in radars])
    return cs.count_cases(np.stack([s["m"] for s in stats]), np.stack([s["n"] for s in stats]), d)


@pytest.mark.parametrize("section", [False, True], ids=["lattice", "section"])
def test_the_tie_scene_holds_ties_of_both_kinds(section):
    scene = cs.tie_scene()
    assert scene.shape == cs.TIE_SHAPE == (3, 9, 21) and scene.n_radars == 5
    a, b = cs.TIE_TWINS
    assert scene.specs[a] == scene.specs[b] and scene.vols[a] is scene.vols[b]
    got = _cases("tie", 0, section)
    print("tie scene,", "section" if section else "lattice", got)
    for key in ("none", "one", "several", "differ", "value_tie", "distance_tie", "distance_tie_other_values"):
        assert got[key] > 0, (key, got)
    if section:
        xs, ys = cs.path("tie")
        assert len(xs) % 4 == 3 and int((xs == 0.0).sum()) >= 4               # points exactly on the mirror column
    else:                                      # the poison reaches voxels, and a NaN of the first radar meets a later number
        assert got["first_radar_nan_yields"] > 0 and got["inf"] > 0, got


def test_the_mirror_radars_tie_exactly_on_the_middle_column():
    scene = cs.tie_scene()
    p, q = cs.TIE_MIRROR
    dp, dq = cs.lattice_d(scene, p), cs.lattice_d(scene, q)
    np.testing.assert_array_equal(dp[:, :, cs.MIRROR_COLUMN], dq[:, :, cs.MIRROR_COLUMN])
    np.testing.assert_array_equal(dp, dq[:, :, ::-1])                    # exact negatives, column for mirrored column
    assert (dp != dq)[:, :, np.arange(21) != cs.MIRROR_COLUMN].all()
    xs, ys = cs.path("tie")
    on = xs == 0.0
    sp, sq = cs.section_d(scene, p, xs, ys), cs.section_d(scene, q, xs, ys)
    np.testing.assert_array_equal(sp[:, on], sq[:, on])
    assert (sp[:, ~on] != sq[:, ~on]).all()
    # the poison is there, unmasked
    dbzh = scene.vols[cs.TIE_POISON].fields["DBZH"]
    live = np.ma.getdata(dbzh)[~np.ma.getmaskarray(dbzh)]
    assert int(np.isnan(live).sum()) == 1 and int(np.isposinf(live).sum()) == 1


@pytest.mark.parametrize("section", [False, True], ids=["lattice", "section"])
def test_scene16_holds_voxels_of_every_kind(section):
    got = _cases("scene16", 0, section)
    print("scene16,", "section" if section else "lattice", got)
    for key in ("none", "one", "several", "differ"):
        assert got[key] > 0, (key, got)
    if section:
        assert len(cs.path("scene16")[0]) % 4 == 3


# ---- 3. the C ABI -------------------------------------------------------------------------------------------------------------
NEW = ("rg_roi_grid_mosaic_combine_f32", "rg_roi_section_mosaic_combine_f32")


def test_new_symbols_are_declared_and_bound():
    header = open(os.path.join(REPO, "include", "radargrid_hip.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t|const char\*)\s+(rg_\w+)\s*\(", header, flags=re.M))
    for name, parent in zip(NEW, ("rg_roi_grid_mosaic_f32", "rg_roi_section_mosaic_f32")):
        assert name in declared and name in _native.SIGNATURES
        restype, argtypes = _native.SIGNATURES[name]
        p_restype, p_argtypes = _native.SIGNATURES[parent]
        # the parent's arguments, then combine and out_radar, then the stream
        assert restype is p_restype and argtypes[:len(p_argtypes) - 1] == p_argtypes[:-1]
        assert len(argtypes) == len(p_argtypes) + 2 and argtypes[-1] is p_argtypes[-1]
    m = re.search(r"typedef enum rg_combine \{(.*?)\} rg_combine;", header, re.S)
    codes = {k: int(v) for k, v in re.findall(r"(RG_COMBINE_\w+)\s*=\s*(\d+)", m.group(1))}
    assert codes == {"RG_COMBINE_MEAN": 0, "RG_COMBINE_MAX": 1, "RG_COMBINE_NEAREST_RADAR": 2}
    assert _native.COMBINES == {"mean": 0, "max": 1, "nearest_radar": 2}
    assert rg.MOSAIC_COMBINES == ("mean", "max", "nearest_radar") and rg.NO_RADAR == cs.NO_RADAR == 255
    lib = rg.load_library(require_device=False)
    assert lib.rg_version() == _native.ABI_VERSION == 104                # functions were added; no signature changed
    assert "#define RG_VERSION 104" in header


def _cells():
    return _native.CellGrid(x0=0.0, y0=0.0, inv_cx=1e-3, inv_cy=1e-3, z_lo=-1e3, z_hi=1e4, ncx=4, ncy=4, levels=0, level0=0)


def _grid_entry(**kw):
    e = _native.MosaicRadar(sorted_gates=P, cell_start=P, xc=P, yc=P, zc=P, ix0=0, iy0=0, nx_win=4, ny_win=4, gate_offset=0,
                            n_gates=10)
    e.cells = _cells()
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def _section_entry(**kw):
    e = _native.SectionRadar(sorted_gates=P, cell_start=P, xs=P, ys=P, zc=P, gate_offset=0, n_gates=10)
    e.cells = _cells()
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def _grid(table, combine, out_radar=None, weighting=0, n_fields=1, stride=1, out=P):
    lib = rg.load_library(require_device=False)
    arr = (_native.MosaicRadar * len(table))(*table)
    return lib.rg_roi_grid_mosaic_combine_f32(arr, len(table), 2, 4, 4, 250.0, 0.01746, weighting, P, n_fields, stride, 10, 0.0,
                                              out, combine, out_radar, None)


def _section(table, combine, out_radar=None, weighting=0, n_fields=1, stride=1, out=P):
    lib = rg.load_library(require_device=False)
    arr = (_native.SectionRadar * len(table))(*table)
    return lib.rg_roi_section_mosaic_combine_f32(arr, len(table), 2, 5, 250.0, 0.01746, weighting, P, n_fields, stride, 10, 0.0,
                                                 out, combine, out_radar, None)


@pytest.mark.parametrize("call, entry, name", [(_grid, _grid_entry, NEW[0]), (_section, _section_entry, NEW[1])],
                         ids=["grid", "section"])
def test_combine_entry_points_refuse_bad_arguments(call, entry, name):
    """Every call carries an entry the table checks refuse (its gates lie past n_gates_total): nothing is ever launched."""
    lib = rg.load_library(require_device=False)
    E = _native
    bad = entry(n_gates=11)
    for code in (3, -1, 255):
        assert call([bad], code) == E.RG_EINVAL
        msg = lib.rg_last_error()
        assert name.encode() in msg and b"unknown combine" in msg, msg
    assert call([bad], E.COMBINES["mean"], out_radar=P) == E.RG_EINVAL
    msg = lib.rg_last_error()
    assert name.encode() in msg and b"out_radar" in msg, msg
    for combine in E.COMBINES.values():
        # the parents' checks, under every rule: the closest-gate mode, the weighting, the fields, the table
        assert call([bad], combine, weighting=E.WEIGHTINGS["closest"]) == E.RG_EUNSUPPORTED
        assert b"closest" in lib.rg_last_error() and name.encode() in lib.rg_last_error()
        assert call([bad], combine, weighting=7) == E.RG_EINVAL and b"unknown weighting" in lib.rg_last_error()
        assert call([bad], combine, n_fields=9, stride=8) == E.RG_EUNSUPPORTED
        assert call([bad], combine, stride=2) == E.RG_EINVAL and b"stride=2" in lib.rg_last_error()
        assert call([bad], combine, out=None) == E.RG_EINVAL
        assert call([bad], combine) == E.RG_EINVAL
        msg = lib.rg_last_error()
        assert b"exceed n_gates_total" in msg and name.encode() in msg, msg
        assert call([entry(), entry(gate_offset=5, n_gates=6)], combine) == E.RG_EINVAL and b"radar 1:" in lib.rg_last_error()
        assert call([entry(cell_start=0), bad], combine) == E.RG_EINVAL and b"null pointer" in lib.rg_last_error()
    for combine in (E.COMBINES["max"], E.COMBINES["nearest_radar"]):         # with a provenance output the checks are the same
        assert call([bad], combine, out_radar=P) == E.RG_EINVAL and b"exceed n_gates_total" in lib.rg_last_error()
    assert call([bad] * (E.RG_MAX_RADARS + 1), 1) == E.RG_EUNSUPPORTED and b"exceeds 16" in lib.rg_last_error()


# ---- 4. the Python surface, without a device -------------------------------------------------------------------------------------
class _NoDevice:
    def __init__(self, shape, limits, window):
        self.full_shape, self.grid_limits, self.window = shape, limits, window

    def __getattr__(self, name):
        raise AssertionError(f"validation touched search.{name}")


class _NoDeviceMosaic(rg.MosaicSearch):
    """A MosaicSearch of stub searches: nothing of it is on a device."""

    def __init__(self, shape, limits, origins):
        self.grid_shape, self.grid_limits = shape, limits
        self.origins = np.asarray(origins, dtype=np.float64)
        self.windows = [(0, shape[1], 0, shape[2])] * len(origins)
        self.searches = [_NoDevice(shape, rg.mosaic_limits(limits, o), w) for o, w in zip(self.origins, self.windows)]
        self.n_gates = [6] * len(origins)
        self.min_radius, self.beam_factor, self.toa = 250.0, 0.01746, 17000.0

    @property
    def dev(self):
        raise AssertionError("validation touched search.dev")


def _stub():
    return _NoDeviceMosaic((3, 5, 9), ((0.0, 2000.0), (-4000.0, 4000.0), (-8000.0, 8000.0)), [(0.0, 0.0, 0.0), (0.0, 500.0, 500.0)])


def _host_geometry(counts):
    g = rg.GridGeometry((1, 2, 3), ((0, 1), (0, 1), (0, 1)), np.zeros(7, dtype=np.int32), np.zeros(0, dtype=np.int32),
                        np.zeros(0, dtype=np.float32), 17000.0)
    g.gate_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    g.origins = np.zeros((len(counts), 3))
    return g


def test_python_validation_happens_before_the_device():
    m = _stub()
    ok = np.float32([0.0, 100.0])
    nothing = [[object()]] * 2                   # never looked at: the combine rule is checked first
    with pytest.raises(ValueError, match="Unknown combine rule: median"):
        rg.mosaic_fields_device(m, nothing, combine="median")
    with pytest.raises(ValueError, match="Unknown combine rule: median"):
        rg.mosaic_section_fields_device(m, ok, ok, nothing, combine="median")
    with pytest.raises(ValueError, match="return_radar needs combine"):
        rg.mosaic_fields_device(m, nothing, return_radar=True)
    with pytest.raises(ValueError, match="return_radar needs combine"):
        rg.mosaic_fields_device(m, nothing, combine="mean", return_radar=True)
    with pytest.raises(ValueError, match="return_radar needs combine"):
        rg.mosaic_section_fields_device(m, ok, ok, nothing, return_radar=True)
    geom = _host_geometry([5, 7])
    for combine in ("max", "nearest_radar"):
        with pytest.raises(ValueError, match="needs a MosaicSearch"):
            rg.mosaic_fields_device(geom, nothing, combine=combine)
        with pytest.raises(ValueError, match="needs a MosaicSearch"):
            rg.mosaic_fields_device(geom, nothing, combine=combine, return_radar=True)
    with pytest.raises(ValueError, match="Unknown combine rule"):
        rg.mosaic_fields_device(geom, nothing, combine="nearest")
    # the convenience: before the path search is built
    f = np.ma.masked_all(8, dtype=np.float32)
    g = np.zeros(8, dtype=np.float32)
    with pytest.raises(ValueError, match="Unknown combine rule: maximum"):
        rg.mosaic_vertical_section([(g, g, g, (0.0, 0.0, 0.0))], [f], [(0.0, 0.0), (1000.0, 0.0)], 100.0, (0.0, 1000.0), 3,
                                   combine="maximum")
    # with a good rule the next check speaks: the defaults are today's path
    with pytest.raises(ValueError, match="fields of 2 radars"):
        rg.mosaic_fields_device(m, [[object()]], combine="max", return_radar=True)
    with pytest.raises(ValueError, match="fields of 2 radars"):
        rg.mosaic_section_fields_device(m, ok, ok, [[object()]], combine="nearest_radar")
    assert mosaic.MOSAIC_COMBINES is rg.MOSAIC_COMBINES and "MOSAIC_COMBINES" in rg.__all__ and "NO_RADAR" in rg.__all__
