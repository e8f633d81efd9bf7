"""A vertical section through a mosaic, CPU side: what the scene of tests/mosaic_section_scenes.py exercises, the NaN
marking of ``mosaic_section_points`` and ``path_reach`` (host code, no device), the argument validation of the Python surface
and of ``rg_roi_section_mosaic_f32`` (every call fails validation before a launch), the struct layout against the header,
and the fixtures g12_mosaic_section_* (tests/golden/make_mosaic_section_golden.py) against the brute-force oracle."""
import ctypes
import os
import re

import numpy as np
import pytest

import mosaic_scenes as ms
import mosaic_section_scenes as mss
import radar_processor_amd as rg
from conftest import GOLDEN, assert_same_to_rounding
from oracle import radar_grid_oracle as oracle
from radar_processor_amd import _native, mosaic

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 12                                  # a 16-byte aligned address that is never dereferenced


# ---- 1. the scene ----------------------------------------------------------------------------------------------------------
def test_scene_properties():
    got = mss.check_properties()             # the floors are asserted there
    assert got["pairs"] > 0 and got["outside_reached"] == 0
    s = ms.scene16()
    assert set(ms.INERT.values()) <= set(s.kinds)                   # every inert kind is present
    assert got["idle_live"], "no live radar without a point of the path: the wave-uniform skip is not exercised"


def test_scene3_is_exact_on_the_lattice():
    s = mss.scene3()
    assert s.shape == ms.SHAPE and s.limits == ms.LIMITS
    xc = np.linspace(s.limits[2][0], s.limits[2][1], s.shape[2], dtype="float32")
    yc = np.linspace(s.limits[1][0], s.limits[1][1], s.shape[1], dtype="float32")
    for r in range(s.n_radars):
        oz, oy, ox = s.origins[r]
        assert float(oy).is_integer() and float(ox).is_integer()
        lim = rg.mosaic_limits(s.limits, s.origins[r])
        # shared lattice coordinates minus the origin ARE the radar's own float32 tables
        np.testing.assert_array_equal(mss.frame(xc, ox), np.linspace(lim[2][0], lim[2][1], s.shape[2], dtype="float32"))
        np.testing.assert_array_equal(mss.frame(yc, oy), np.linspace(lim[1][0], lim[1][1], s.shape[1], dtype="float32"))
        assert s.window(r) != (0, 0, 0, 0)


# ---- 2. mosaic_section_points -----------------------------------------------------------------------------------------------
class _NoDevice:
    """Stands in for a RoiSearch: the attributes the validation reads; anything else -- the device tensors -- raises."""

    def __init__(self, shape, limits, window):
        self.full_shape = shape
        self.grid_limits = limits
        self.window = window

    def __getattr__(self, name):
        raise AssertionError(f"validation touched search.{name}")


class _NoDeviceMosaic(rg.MosaicSearch):
    """A MosaicSearch of stub searches: nothing of it is on a device."""

    def __init__(self, shape, limits, origins, windows):
        self.grid_shape, self.grid_limits = shape, limits
        self.origins = np.asarray(origins, dtype=np.float64)
        self.windows = list(windows)
        self.searches = [None if w is None else _NoDevice(shape, rg.mosaic_limits(limits, o), w)
                         for o, w in zip(self.origins, windows)]
        self.n_gates = [6] * len(windows)
        self.min_radius, self.beam_factor, self.toa = 250.0, 0.01746, 17000.0

    @property
    def dev(self):
        raise AssertionError("validation touched search.dev")


SHAPE = (3, 5, 9)
LIMITS = ((0.0, 2000.0), (-4000.0, 4000.0), (-8000.0, 8000.0))      # 2 km rows and columns


def _stub():
    # radar 0: the whole grid; radar 1 at (oy, ox) = (1000.5, -3000.25): columns 2 .. 6, rows 1 .. 2; radar 2: no search
    return _NoDeviceMosaic(SHAPE, LIMITS, [(0.0, 0.0, 0.0), (120.0, 1000.5, -3000.25), (0.0, 500.0, 500.0)],
                           [(0, 5, 0, 9), (1, 3, 2, 7), None])


def test_points_in_every_radars_frame():
    m = _stub()
    xs = np.float32([-8000.0, -4000.0, -3999.5, 0.1, 4000.0, 4000.5, 8000.0])
    ys = np.float32([-4000.0, -2000.0, -2000.0, -0.3, 0.0, 0.0, 4000.0])
    pts = rg.mosaic_section_points(m, xs, ys)
    assert len(pts) == 3 and all(a.dtype == b.dtype == np.float32 and a.shape == b.shape == xs.shape for a, b in pts)
    np.testing.assert_array_equal(pts[0][0], xs)                    # origin 0: the points themselves, none outside
    np.testing.assert_array_equal(pts[0][1], ys)
    # radar 1: fl32(f64(x) - ox); inside exactly where the shifted point lies inside its window's float32 table range
    x1 = (xs.astype(np.float64) + 3000.25).astype(np.float32)
    y1 = (ys.astype(np.float64) - 1000.5).astype(np.float32)
    lim = rg.mosaic_limits(LIMITS, (120.0, 1000.5, -3000.25))
    xc = np.linspace(lim[2][0], lim[2][1], 9, dtype="float32")[2:7]
    yc = np.linspace(lim[1][0], lim[1][1], 5, dtype="float32")[1:3]
    inside = (x1 >= xc[0]) & (x1 <= xc[-1]) & (y1 >= yc[0]) & (y1 <= yc[-1])
    assert inside.tolist() == [False, True, True, True, True, False, False]      # both rims of the window are inside
    np.testing.assert_array_equal(pts[1][0], np.where(inside, x1, np.float32(np.nan)))
    np.testing.assert_array_equal(pts[1][1], np.where(inside, y1, np.float32(np.nan)))
    assert float(pts[1][0][3]) == float(np.float32(0.1 + 3000.25)) != 0.1 + 3000.25    # rounded once, from float64
    # a radar without a search: NaN everywhere
    assert np.isnan(pts[2][0]).all() and np.isnan(pts[2][1]).all()


def test_point_validation_happens_before_the_device():
    m = _stub()
    ok = np.float32([0.0, 100.0])
    cases = [
        (np.float32([0.0, 8000.5]), ok, "point 1 .*outside the rectangle"),
        (ok, np.float32([-4000.5, 0.0]), "point 0 .*outside the rectangle"),
        (np.float32([0.0, np.nan]), ok, "finite"),
        (ok, np.float32([np.inf, 0.0]), "finite"),
        (np.zeros(0, np.float32), np.zeros(0, np.float32), "n_points == 0"),
        (ok, np.float32([0.0]), "equal length"),
        (np.zeros((2, 2), np.float32), np.zeros((2, 2), np.float32), "one-dimensional"),
    ]
    for xs, ys, what in cases:
        with pytest.raises(ValueError, match=what):
            rg.mosaic_section_points(m, xs, ys)
        with pytest.raises(ValueError, match=what):
            rg.mosaic_section_fields_device(m, xs, ys, [[object()]] * 3)
        if "outside" not in what:            # the geometry route builds its rectangle from the points: none is outside
            with pytest.raises(ValueError, match=what):
                rg.compute_mosaic_section_geometry([_radar()], xs, ys, (0.0, 1000.0), 3)
    with pytest.raises(ValueError, match="closest"):
        rg.mosaic_section_fields_device(m, ok, ok, [[object()]] * 3, weighting="closest")
    with pytest.raises(ValueError, match="Unknown weighting"):
        rg.mosaic_section_fields_device(m, ok, ok, [[object()]] * 3, weighting="gauss")
    with pytest.raises(TypeError):
        rg.mosaic_section_fields_device(object(), ok, ok, [[object()]])
    with pytest.raises(ValueError, match="distinct indices"):
        rg.mosaic_section_fields_device(m, ok, ok, [[object()]], radars=[3])
    with pytest.raises(ValueError, match="fields of 3 radars"):
        rg.mosaic_section_fields_device(m, ok, ok, [[object()]])
    with pytest.raises(ValueError, match="no fields"):
        rg.mosaic_section_fields_device(m, ok, ok, [[], [], []])


def _radar(n=8, origin=(0.0, 0.0, 0.0)):
    g = np.zeros(n, dtype=np.float32)
    return (g, g, g, origin)


def test_field_validation_happens_before_the_device():
    torch = pytest.importorskip("torch")
    m = _stub()
    ok = np.float32([0.0, 100.0])
    f6, f5 = torch.zeros(6), torch.zeros(5)
    with pytest.raises(ValueError, match="radar 1 field 0: 5 values for 6 gates"):
        rg.mosaic_section_fields_device(m, ok, ok, [[f6], [f5], [f6]])
    with pytest.raises(ValueError, match="radar 2 field 0: 5 values"):
        rg.mosaic_section_fields_device(m, ok, ok, [[f5]], radars=[2])
    with pytest.raises(ValueError, match="one entry per radar"):
        rg.mosaic_section_fields_device(m, ok, ok, [[f6]] * 3, shared_masks=[None])
    with pytest.raises(_native.NativeUnavailable, match="device-resident"):
        rg.mosaic_section_fields_device(m, ok, ok, [[f6]] * 3)      # host tensors: refused, the search's device not read


def test_geometry_and_convenience_validation_happens_before_the_device():
    line = [(0.0, 0.0), (1000.0, 0.0)]
    ok = np.float32([0.0, 100.0])
    f = np.ma.masked_all(8, dtype=np.float32)
    with pytest.raises(ValueError, match="closest"):
        rg.compute_mosaic_section_geometry([_radar()], ok, ok, (0.0, 1000.0), 3, weighting="closest")
    with pytest.raises(ValueError, match="Unknown weighting"):
        rg.compute_mosaic_section_geometry([_radar()], ok, ok, (0.0, 1000.0), 3, weighting="gauss")
    with pytest.raises(ValueError, match="at least one radar"):
        rg.compute_mosaic_section_geometry([], ok, ok, (0.0, 1000.0), 3)
    with pytest.raises(ValueError, match="origin must be"):
        rg.compute_mosaic_section_geometry([_radar(origin=(0.0, np.nan, 0.0))], ok, ok, (0.0, 1000.0), 3)
    with pytest.raises(ValueError, match="nz must be"):
        rg.compute_mosaic_section_geometry([_radar()], ok, ok, (0.0, 1000.0), 0)
    with pytest.raises(ValueError, match="finite"):
        rg.compute_mosaic_section_geometry([_radar()], np.float32([0.0, np.nan]), ok, (0.0, 1000.0), 3)
    with pytest.raises(ValueError, match="at most 16"):
        rg.MosaicSearch.for_path([_radar()] * 17, ok, ok, (0.0, 1000.0), 3)
    with pytest.raises(ValueError, match="nz must be"):
        rg.MosaicSearch.for_path([_radar()], ok, ok, (0.0, 1000.0), 0)
    with pytest.raises(ValueError, match="equal length"):
        rg.MosaicSearch.for_path([_radar()], ok, ok[:1], (0.0, 1000.0), 3)
    with pytest.raises(ValueError, match="at least two"):
        rg.mosaic_vertical_section([_radar()], [f], [(0.0, 0.0)], 100.0, (0.0, 1000.0), 3)
    with pytest.raises(ValueError, match="positive"):
        rg.mosaic_vertical_section([_radar()], [f], line, 0.0, (0.0, 1000.0), 3)
    with pytest.raises(ValueError, match="closest"):
        rg.mosaic_vertical_section([_radar()], [f], line, 100.0, (0.0, 1000.0), 3, weighting="closest")
    with pytest.raises(ValueError, match="one field and one filter list per radar"):
        rg.mosaic_vertical_section([_radar(), _radar()], [f], line, 100.0, (0.0, 1000.0), 3)
    with pytest.raises(ValueError, match="radar 0 has 8 gates, its field 5"):
        rg.mosaic_vertical_section([_radar()], [f[:5]], line, 100.0, (0.0, 1000.0), 3)
    with pytest.raises(ValueError, match="at most 16"):
        rg.mosaic_vertical_section([_radar()] * 17, [f] * 17, line, 100.0, (0.0, 1000.0), 3)


# ---- 3. path_reach -----------------------------------------------------------------------------------------------------------
def test_path_reach():
    # a small radar: gates within 3 km of the antenna, up to 1 km above it
    rng = np.random.default_rng(3)
    gx = np.float32(rng.uniform(-3e3, 3e3, 200))
    gy = np.float32(rng.uniform(-3e3, 3e3, 200))
    gz = np.float32(rng.uniform(0.0, 1e3, 200))
    box = (-20e3, 20e3, -10e3, 10e3)                                # (x_min, x_max, y_min, y_max) of a path
    kw = dict(min_radius=250.0, beam_factor=0.01746, toa=17000.0)
    # strictly inside the path's box -- between the two columns of a 2 x 2 lattice over it, whose reach window is empty
    assert rg.path_reach(gx, gy, gz, (0.0, 1e3, -2e3), box, **kw)
    assert rg.reach_window(gx, gy, gz, (3, 2, 2), ((0.0, 5e3), box[2:], box[:2]), (0.0, 1e3, -2e3), **kw) == (0, 0, 0, 0)
    # beyond it on every side: R_g = max(250, 0.01746 |g| / (1 - 0.01746)) is 250 m here
    reach = 3e3 + 250.0 * (1.0 + 1e-9) + 1e-6
    for oy, ox in ((0.0, 20e3 + reach + 1.0), (0.0, -20e3 - reach - 1.0), (10e3 + reach + 1.0, 0.0), (-10e3 - reach - 1.0, 0.0)):
        assert not rg.path_reach(gx, gy, gz, (0.0, oy, ox), box, **kw)
    assert rg.path_reach(gx, gy, gz, (0.0, 0.0, 20e3 + 3e3), box, **kw)          # its gates still overlap the rim
    # a degenerate rectangle (a path along an axis) is legal
    assert rg.path_reach(gx, gy, gz, (0.0, 0.0, 0.0), (-5e3, 5e3, 0.0, 0.0), **kw)
    # an antenna above toa: every gate is cut
    assert not rg.path_reach(gx, gy, gz, (17000.0 + 1.0, 1e3, -2e3), box, **kw)
    assert rg.path_reach(gx, gy, gz, (17000.0 - 500.0, 1e3, -2e3), box, **kw)    # ... some gates below the cut
    # no gates; a beam factor outside [0, 1): no bound
    assert not rg.path_reach(gx[:0], gy[:0], gz[:0], (0.0, 0.0, 0.0), box, **kw)
    assert rg.path_reach(gx, gy, gz, (0.0, 0.0, 1e6), box, min_radius=250.0, beam_factor=1.0, toa=17000.0)
    with pytest.raises(ValueError, match="rectangle"):
        rg.path_reach(gx, gy, gz, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="origin"):
        rg.path_reach(gx, gy, gz, (0.0, 0.0), box)


def test_path_reach_is_conservative_on_the_scene():
    s = ms.scene16()
    xs, ys, _ = mss.path()
    box = (float(xs.min()), float(xs.max()), float(ys.min()), float(ys.max()))
    for r in range(s.n_radars):
        v = s.vols[r]
        reaches = rg.path_reach(v.gate_x, v.gate_y, v.gate_z, s.origins[r], box, s.min_radius, s.beam_factor, s.toa)
        assert reaches or mss.radar_pairs(s, r)[0][-1] == 0, r
        if s.kinds[r] in ("far", "no_gates", "above_toa"):
            assert not reaches, (r, s.kinds[r])


# ---- 4. the C ABI ------------------------------------------------------------------------------------------------------------
def test_section_radar_layout_matches_the_header():
    header = open(os.path.join(REPO, "include", "radargrid_hip.h")).read()
    body = re.search(r"typedef struct rg_section_radar \{(.*?)\} rg_section_radar;", header, re.S).group(1)
    names = re.findall(r"\*?\s*(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    R = _native.SectionRadar
    assert names == [n for n, _ in R._fields_]
    assert ctypes.sizeof(R) == 120                  # 64-bit pointers, a 64-byte rg_cellgrid, three pointers, two int64
    assert [getattr(R, n).offset for n, _ in R._fields_] == [0, 8, 16, 80, 88, 96, 104, 112]
    # rg_mosaic_radar is untouched
    assert ctypes.sizeof(_native.MosaicRadar) == 136
    assert "rg_roi_section_mosaic_f32" in _native.SIGNATURES


def _entry(**kw):
    e = _native.SectionRadar(sorted_gates=P, cell_start=P, xs=P, ys=P, zc=P, gate_offset=0, n_gates=10)
    e.cells = _native.CellGrid(x0=0.0, y0=0.0, inv_cx=1e-3, inv_cy=1e-3, z_lo=-1e3, z_hi=1e4, ncx=4, ncy=4, levels=0,
                               level0=0)
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def _call(table, n_radars=None, nz=2, n_points=5, weighting=0, packed=P, n_fields=1, stride=1, n_total=10, out=P):
    lib = rg.load_library(require_device=False)
    arr = None
    if table is not None:
        arr = (_native.SectionRadar * len(table))(*table)
        n_radars = len(table) if n_radars is None else n_radars
    return lib.rg_roi_section_mosaic_f32(arr, n_radars or 0, nz, n_points, 250.0, 0.01746, weighting, packed, n_fields,
                                         stride, n_total, 0.0, out, None)


def test_entry_point_argument_validation():
    """Every call carries an entry the checks refuse (its gates lie past n_gates_total): nothing is ever launched."""
    lib = rg.load_library(require_device=False)
    E = _native
    bad = _entry(n_gates=11)
    assert _call(None, 1) == E.RG_EINVAL and b"null radar table" in lib.rg_last_error()
    assert _call([bad], n_radars=0) == E.RG_EINVAL
    assert _call([bad], n_radars=-1) == E.RG_EINVAL
    assert _call([bad] * (E.RG_MAX_RADARS + 1)) == E.RG_EUNSUPPORTED and b"exceeds 16" in lib.rg_last_error()
    assert _call([bad], nz=0) == E.RG_EINVAL and b"bad section shape" in lib.rg_last_error()
    assert _call([bad], n_points=0) == E.RG_EINVAL
    assert _call([bad], n_points=-3) == E.RG_EINVAL
    assert _call([bad], stride=2) == E.RG_EINVAL and b"stride=2" in lib.rg_last_error()
    assert _call([bad], n_fields=3, stride=2) == E.RG_EINVAL
    assert _call([bad], n_fields=9, stride=8) == E.RG_EUNSUPPORTED
    assert _call([bad], n_fields=0) == E.RG_EUNSUPPORTED
    assert _call([bad], weighting=E.WEIGHTINGS["closest"]) == E.RG_EUNSUPPORTED and b"closest" in lib.rg_last_error()
    assert _call([bad], weighting=7) == E.RG_EINVAL and b"unknown weighting" in lib.rg_last_error()
    assert _call([bad], weighting=-1) == E.RG_EINVAL
    assert _call([bad], packed=P + 4) == E.RG_EALIGN and b"packed" in lib.rg_last_error()
    assert _call([bad], packed=None) == E.RG_EINVAL
    assert _call([bad], out=None) == E.RG_EINVAL
    assert _call([bad], n_total=2 ** 31) == E.RG_EUNSUPPORTED and b"n_gates_total" in lib.rg_last_error()
    assert _call([bad], n_total=-1) == E.RG_EUNSUPPORTED
    # 2^31 - 1 points x 40 levels: the wave count does not fit 32 bits
    assert _call([bad], nz=40, n_points=2 ** 31 - 1) == E.RG_EUNSUPPORTED and b"too large" in lib.rg_last_error()
    # the gate range of every entry must lie inside the packed fields
    assert _call([bad]) == E.RG_EINVAL and b"exceed n_gates_total" in lib.rg_last_error()
    assert _call([_entry(), _entry(gate_offset=5, n_gates=6)]) == E.RG_EINVAL and b"radar 1:" in lib.rg_last_error()
    assert _call([_entry(gate_offset=-1, n_gates=1), bad]) == E.RG_EINVAL and b"radar 0:" in lib.rg_last_error()
    assert _call([_entry(n_gates=-1), bad]) == E.RG_EINVAL
    # an entry that takes part needs its search structure, its points and its levels
    for name in ("cell_start", "xs", "ys", "zc"):
        assert _call([_entry(**{name: 0}), bad]) == E.RG_EINVAL and b"null pointer" in lib.rg_last_error(), name
    assert _call([_entry(sorted_gates=P + 8), bad]) == E.RG_EALIGN and b"sorted_gates" in lib.rg_last_error()
    e = _entry()
    e.cells.ncx = 0
    assert _call([e, bad]) == E.RG_EINVAL and b"bad cell grid" in lib.rg_last_error()
    e = _entry()
    e.cells.levels, e.cells.level0 = 3, 2                            # levels 2 .. 3 of 3
    assert _call([e, bad]) == E.RG_EINVAL and b"per-level" in lib.rg_last_error()
    # ... an entry without gates, or without a search structure, does not: none of its pointers is read
    for idle in (_entry(n_gates=0, cell_start=0, xs=0, ys=0, zc=0), _entry(sorted_gates=0, cell_start=0, xs=0, ys=0, zc=0)):
        assert _call([idle, bad]) == E.RG_EINVAL and b"radar 1: gates 0 + 11 exceed" in lib.rg_last_error()
    # the last slot of a full table is checked like the first
    good = [_entry(gate_offset=k % 3, n_gates=7) for k in range(15)]
    assert _call(good + [_entry(gate_offset=5, n_gates=6)]) == E.RG_EINVAL and b"radar 15:" in lib.rg_last_error()
    assert lib.rg_version() == E.ABI_VERSION == 104                  # a function was added; no signature changed


def test_names_are_exported():
    for name in ("mosaic_section_points", "path_reach", "mosaic_section_fields_device", "compute_mosaic_section_geometry",
                 "mosaic_vertical_section"):
        assert name in rg.__all__ and callable(getattr(rg, name))
    assert callable(rg.MosaicSearch.for_path) and callable(rg.MosaicSearch.section_table)
    assert mosaic.mosaic_section_points is rg.mosaic_section_points


# ---- 5. the fixtures against the brute-force oracle ---------------------------------------------------------------------------
def test_fixtures_are_small_and_complete():
    s = ms.scene16()
    xs, ys, dist = mss.path()
    for w in mss.WEIGHTINGS:
        assert os.path.getsize(os.path.join(GOLDEN, f"g12_mosaic_section_{w}.npz")) < 1_000_000
        meta, arrays = mss.fixture(w)
        assert meta["case"] == "G12" and meta["weighting"] == w and meta["scene"] == "scene16"
        assert meta["digests"] == [v.digest() for v in s.vols]
        assert meta["origins"] == [list(o) for o in s.origins]
        assert meta["vertices"] == [list(v) for v in mss.VERTICES] and meta["spacing"] == mss.SPACING
        assert meta["nz"] == s.shape[0] and meta["toa"] == s.toa and meta["min_radius"] == s.min_radius
        assert meta["fields"] == list(mss.FIELDS) and meta["qc"] == list(mss.QC) and meta["fill_value"] == mss.FILL
        np.testing.assert_array_equal(arrays["xs"], xs)
        np.testing.assert_array_equal(arrays["ys"], ys)
        np.testing.assert_array_equal(arrays["s"], dist)
        lengths = np.diff(arrays["indptr"].astype(np.int64))
        assert len(lengths) == s.shape[0] * mss.N_POINTS and meta["report"]["pairs"] == int(lengths.sum())
        assert (lengths > 0).mean() >= 0.25 and lengths.max() > 256
        for f in mss.FIELDS:
            assert {f"grid_{f}", f"grid_{f}_qc", f"grid_{f}_qc_fill"} <= set(arrays)


def test_brute_force_reproduces_the_reference():
    """Neighbour sets exactly; weights to <= 1 ulp for Barnes (two exp implementations) and exactly for the others; the
    reference's apply on its rows against the oracle's on the brute-force rows, and within the float64 bound."""
    s = ms.scene16()
    shape = (s.shape[0], 1, mss.N_POINTS)
    for weighting in mss.WEIGHTINGS:
        _, ref = mss.fixture(weighting)
        ip, idx, w = mss.mosaic_csr(s, weighting, exact=False)
        _, _, w64 = mss.mosaic_csr(s, weighting)
        c_ip, c_idx, c_w = oracle.canonical_rows(ip, idx, w)
        r_ip, r_idx, r_w = oracle.canonical_rows(ref["indptr"], ref["gate_indices"], ref["weights"])
        np.testing.assert_array_equal(c_ip, r_ip)
        np.testing.assert_array_equal(c_idx, r_idx)
        if weighting == "barnes2":
            ulp = np.abs(c_w.view(np.int32).astype(np.int64) - r_w.view(np.int32).astype(np.int64))
            assert ulp.max(initial=0) <= 1
        else:
            np.testing.assert_array_equal(c_w, r_w)
        for f in mss.FIELDS:
            data, mask = mss.concat_field(s, f)
            _, mask_qc = mss.concat_field(s, f, qc=True)
            scale = float(np.nanmax(np.abs(data[~mask])))
            assert_same_to_rounding(oracle.csr_apply(ip, idx, w, data, mask, shape), ref[f"grid_{f}"], scale)
            assert_same_to_rounding(oracle.csr_apply(ip, idx, w, data, mask_qc, shape), ref[f"grid_{f}_qc"], scale)
            assert_same_to_rounding(oracle.csr_apply(ip, idx, w, data, mask_qc, shape, fill_value=mss.FILL),
                                    ref[f"grid_{f}_qc_fill"], scale, fill=mss.FILL)
            stats = oracle.voxel_stats(ip, idx, w64, data, mask_qc)
            assert oracle.bound_ratio(ref[f"grid_{f}_qc"], stats, oracle.DELTA_CSR[weighting]).max(initial=0.0) <= 1.0
