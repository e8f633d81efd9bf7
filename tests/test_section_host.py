"""Vertical cross-sections, CPU side: ``section_path`` against known answers, the argument validation of the Python surface
(which happens before any device is touched) and of the three C entry points (every call here fails validation before a
launch), and the brute-force float64 restatement of tests/section_scenes.py against the reference's fixtures
(g11_section_*, built by tests/golden/make_section_golden.py)."""
import os

import numpy as np
import pytest

import radar_processor_amd as rg
import section_scenes as sc
from conftest import GOLDEN, assert_same_to_rounding
from oracle import radar_grid_oracle as oracle
from radar_processor_amd import _native, section

P = 1 << 12                                  # a 16-byte aligned address that is never dereferenced


# ---- 1. section_path ---------------------------------------------------------------------------------------------------
def test_section_path_known_answers():
    # 3-4-5 segment, then 6 m straight up: L = 11
    xs, ys, s = rg.section_path([(0.0, 0.0), (3.0, 4.0), (3.0, 10.0)], 2.5)
    assert xs.dtype == ys.dtype == np.float32 and s.dtype == np.float64
    np.testing.assert_array_equal(s, [0.0, 2.5, 5.0, 7.5, 10.0])            # j = 0 .. floor(11 / 2.5) = 4
    np.testing.assert_array_equal(xs, np.float32([0.0, 1.5, 3.0, 3.0, 3.0]))
    np.testing.assert_array_equal(ys, np.float32([0.0, 2.0, 4.0, 6.5, 9.0]))  # the vertex is a sample; the end is not
    # the end is a sample exactly where L is a multiple of the spacing
    xs, ys, s = rg.section_path([(0.0, 0.0), (3.0, 4.0), (3.0, 10.0)], 5.5)
    np.testing.assert_array_equal(s, [0.0, 5.5, 11.0])
    np.testing.assert_array_equal(xs, np.float32([0.0, 3.0, 3.0]))
    np.testing.assert_array_equal(ys, np.float32([0.0, 4.5, 10.0]))
    # a spacing longer than the path: the first vertex alone
    xs, ys, s = rg.section_path([(7.0, -2.0), (8.0, -2.0)], 3.0)
    assert xs.tolist() == [7.0] and ys.tolist() == [-2.0] and s.tolist() == [0.0]


def test_section_path_rounds_once_from_float64():
    v = [(0.1, 0.2), (1000.1, 300.2)]
    xs, ys, s = rg.section_path(v, 7.0)
    L = np.hypot(1000.0, 300.0)
    assert len(s) == int(np.floor(L / 7.0)) + 1 == 150
    t = s / L
    np.testing.assert_array_equal(xs, (0.1 + t * (1000.1 - 0.1)).astype(np.float32))
    np.testing.assert_array_equal(ys, (0.2 + t * (300.2 - 0.2)).astype(np.float32))
    assert xs[0] == np.float32(0.1) and float(xs[0]) != 0.1                    # float32 values, not float64 ones


def test_section_path_of_the_fixture_scene():
    for name, n in (("diag", 524), ("dogleg", 610)):
        xs, ys, s = sc.path_points(name)
        assert len(xs) == len(ys) == len(s) == n
        assert s[1] - s[0] == sc.PATHS[name][1]


@pytest.mark.parametrize("vertices, spacing, what", [
    ([(0.0, 0.0)], 1.0, "at least two"),
    ([], 1.0, "at least two"),
    ([(0.0, 0.0, 0.0), (1.0, 1.0, 1.0)], 1.0, "at least two"),
    ([(0.0, 0.0), (1.0, 1.0), (1.0, 1.0)], 1.0, "zero length"),
    ([(0.0, 0.0), (1.0, 1.0)], 0.0, "positive"),
    ([(0.0, 0.0), (1.0, 1.0)], -2.0, "positive"),
    ([(0.0, 0.0), (np.nan, 1.0)], 1.0, "finite"),
    ([(0.0, 0.0), (np.inf, 1.0)], 1.0, "finite"),
    ([(0.0, 0.0), (1.0, 1.0)], np.nan, "finite"),
    ([(0.0, 0.0), (1.0, 1.0)], np.inf, "finite"),
])
def test_section_path_refusals(vertices, spacing, what):
    with pytest.raises(ValueError, match=what):
        rg.section_path(vertices, spacing)


# ---- 2. validation before any device use -------------------------------------------------------------------------------
class _NoDevice:
    """Stands in for a RoiSearch: the attributes the validation reads; anything else -- the device tensors -- raises."""

    def __init__(self, shape=(3, 5, 9), limits=((0.0, 2000.0), (-4000.0, 4000.0), (-8000.0, 8000.0)), window=None):
        self.full_shape = shape
        self.grid_limits = limits
        self.window = window or (0, shape[1], 0, shape[2])
        self.grid_shape = (shape[0], self.window[1] - self.window[0], self.window[3] - self.window[2])
        self.n_gates = 6

    def __getattr__(self, name):
        raise AssertionError(f"validation touched search.{name}")


def _device_calls(search, xs, ys, **kw):
    return [lambda: rg.section_fields_device(search, xs, ys, [object()], **kw),
            lambda: rg.compute_section_geometry(search, xs, ys, **kw)]


def test_section_rectangle():
    assert rg.section_rectangle(_NoDevice()) == (-8000.0, 8000.0, -4000.0, 4000.0)
    # a windowed search: the window's coordinate range (slices of the whole grid's float32 tables)
    w = _NoDevice(window=(1, 3, 2, 7))
    yc = np.linspace(-4000.0, 4000.0, 5, dtype="float32")
    xc = np.linspace(-8000.0, 8000.0, 9, dtype="float32")
    assert rg.section_rectangle(w) == (float(xc[2]), float(xc[6]), float(yc[1]), float(yc[2]))
    # limits that float32 rounds: the rectangle is the rounded table's
    r = rg.section_rectangle(_NoDevice(limits=((0.0, 1.0), (0.1, 0.7), (-0.3, 16777217.0))))
    assert r == (float(np.float32(-0.3)), 16777216.0, float(np.float32(0.1)), float(np.float32(0.7)))


def test_point_validation_happens_before_the_device():
    s = _NoDevice()
    ok = np.float32([0.0, 100.0])
    cases = [
        (np.float32([0.0, 8000.5]), ok, "point 1 .*outside the rectangle"),
        (np.float32([-8001.0, 0.0]), ok, "point 0 .*outside the rectangle"),
        (ok, np.float32([0.0, 4000.5]), "point 1 .*outside the rectangle"),
        (ok, np.float32([-4000.5, 0.0]), "point 0 .*outside the rectangle"),
        (np.float32([0.0, np.nan]), ok, "finite"),
        (ok, np.float32([np.inf, 0.0]), "finite"),
        (np.float32([-np.inf, 0.0]), ok, "finite"),
        (np.zeros(0, np.float32), np.zeros(0, np.float32), "n_points == 0"),
        (ok, np.float32([0.0]), "equal length"),
        (np.zeros((2, 2), np.float32), np.zeros((2, 2), np.float32), "one-dimensional"),
    ]
    for xs, ys, what in cases:
        for call in _device_calls(s, xs, ys):
            with pytest.raises(ValueError, match=what):
                call()
    for call in _device_calls(s, ok, ok, weighting="closest"):
        with pytest.raises(ValueError, match="closest"):
            call()
    for call in _device_calls(s, ok, ok, weighting="gauss"):
        with pytest.raises(ValueError, match="Unknown weighting"):
            call()
    # the rim of the rectangle is inside; a windowed search takes the window's range
    w = _NoDevice(window=(1, 3, 2, 7))
    xs, ys = section._check_points(w, [-4000.0, 4000.0], [-2000.0, 0.0], "nearest")
    assert xs.dtype == ys.dtype == np.float32 and xs.tolist() == [-4000.0, 4000.0] and ys.tolist() == [-2000.0, 0.0]
    for call in _device_calls(w, np.float32([4000.5]), np.float32([0.0])):
        with pytest.raises(ValueError, match="outside the rectangle"):
            call()
    for call in _device_calls(w, np.float32([0.0]), np.float32([2000.0])):
        with pytest.raises(ValueError, match="outside the rectangle"):
            call()
    with pytest.raises(ValueError, match="no fields"):
        rg.section_fields_device(s, ok, ok, [])


def test_field_validation_happens_before_the_device():
    torch = pytest.importorskip("torch")

    class WithDevice(_NoDevice):
        dev = torch.device("cuda", 0)

    s = WithDevice()
    ok = np.float32([0.0, 100.0])
    with pytest.raises(ValueError, match="field 0: expected a contiguous float32 tensor of 6 gates"):
        rg.section_fields_device(s, ok, ok, [torch.zeros(6)])               # a host tensor


def test_vertical_section_validation_happens_before_the_device():
    g = np.zeros(4, dtype=np.float32)
    f = np.ma.masked_all(4, dtype=np.float32)
    line = [(0.0, 0.0), (1000.0, 0.0)]
    with pytest.raises(ValueError, match="at least two"):
        rg.vertical_section(g, g, g, f, [(0.0, 0.0)], 100.0, (0.0, 1000.0), 3)
    with pytest.raises(ValueError, match="positive"):
        rg.vertical_section(g, g, g, f, line, 0.0, (0.0, 1000.0), 3)
    with pytest.raises(ValueError, match="closest"):
        rg.vertical_section(g, g, g, f, line, 100.0, (0.0, 1000.0), 3, weighting="closest")
    with pytest.raises(ValueError, match="Unknown weighting"):
        rg.vertical_section(g, g, g, f, line, 100.0, (0.0, 1000.0), 3, weighting="gauss")
    with pytest.raises(ValueError, match="nz must be"):
        rg.vertical_section(g, g, g, f, line, 100.0, (0.0, 1000.0), 0)
    with pytest.raises(ValueError, match="additional_filters"):
        rg.vertical_section(g, g, g, f, line, 100.0, (0.0, 1000.0), 3, additional_filters="RHOHV")


def test_names_are_exported():
    for name in ("section_path", "section_rectangle", "section_fields_device", "compute_section_geometry",
                 "vertical_section"):
        assert name in rg.__all__ and callable(getattr(rg, name))


# ---- 3. the C ABI ------------------------------------------------------------------------------------------------------
def _cells(**kw):
    c = dict(x0=0.0, y0=0.0, inv_cx=1e-3, inv_cy=1e-3, z_lo=-1e3, z_hi=1e4, ncx=4, ncy=4, levels=0, level0=0)
    c.update(kw)
    return _native.CellGrid(**c)


def _grid(lib, sorted_gates=P, cell_start=P, cells="default", xs=P, ys=P, zc=P, nz=2, n_points=5, weighting=0, packed=P,
          n_fields=1, stride=1, out=P):
    cells = _cells() if cells == "default" else cells
    return lib.rg_roi_section_f32(sorted_gates, cell_start, cells, xs, ys, zc, nz, n_points, 250.0, 0.01746, weighting,
                                  packed, n_fields, stride, 0.0, out, None)


def _count(lib, sorted_gates=P, cell_start=P, cells="default", xs=P, ys=P, zc=P, nz=2, n_points=5, counts=P):
    cells = _cells() if cells == "default" else cells
    return lib.rg_section_count_f32(sorted_gates, cell_start, cells, xs, ys, zc, nz, n_points, 250.0, 0.01746, counts, None)


def _fill(lib, sorted_gates=P, cell_start=P, cells="default", xs=P, ys=P, zc=P, nz=2, n_points=5, weighting=0, indptr=P,
          gate_idx=P, weights=P):
    cells = _cells() if cells == "default" else cells
    return lib.rg_section_fill_f32(sorted_gates, cell_start, cells, xs, ys, zc, nz, n_points, 250.0, 0.01746, weighting,
                                   indptr, gate_idx, weights, None)


def test_section_entry_points_refuse_bad_arguments():
    """Every call carries an argument the host-side checks refuse: nothing is launched, no device is needed."""
    lib = rg.load_library(require_device=False)
    E = _native
    for call in (_grid, _count, _fill):
        for name in ("sorted_gates", "cell_start", "cells", "xs", "ys", "zc"):
            assert call(lib, **{name: None}) == E.RG_EINVAL, (call.__name__, name)
            assert b"null" in lib.rg_last_error()
        assert call(lib, nz=0) == E.RG_EINVAL and b"bad section shape" in lib.rg_last_error()
        assert call(lib, n_points=0) == E.RG_EINVAL
        assert call(lib, n_points=-3) == E.RG_EINVAL
        assert call(lib, sorted_gates=P + 8) == E.RG_EALIGN and b"sorted_gates" in lib.rg_last_error()
        assert call(lib, cells=_cells(ncx=0)) == E.RG_EINVAL and b"bad cell grid" in lib.rg_last_error()
        assert call(lib, cells=_cells(levels=3, level0=2)) == E.RG_EINVAL          # levels 2 .. 3 of 3
        # 2^31 - 1 points x 40 levels: the wave count does not fit 32 bits
        assert call(lib, nz=40, n_points=2 ** 31 - 1) == E.RG_EUNSUPPORTED and b"too large" in lib.rg_last_error()
    for name in ("packed", "out"):
        assert _grid(lib, **{name: None}) == E.RG_EINVAL
    assert _count(lib, counts=None) == E.RG_EINVAL
    for name in ("indptr", "gate_idx", "weights"):
        assert _fill(lib, **{name: None}) == E.RG_EINVAL
    for call in (_grid, _fill):
        assert call(lib, weighting=E.WEIGHTINGS["closest"]) == E.RG_EUNSUPPORTED and b"closest" in lib.rg_last_error()
        assert call(lib, weighting=4) == E.RG_EINVAL and b"unknown weighting" in lib.rg_last_error()
        assert call(lib, weighting=-1) == E.RG_EINVAL
    assert _grid(lib, n_fields=9, stride=8) == E.RG_EUNSUPPORTED
    assert _grid(lib, n_fields=0) == E.RG_EUNSUPPORTED
    assert _grid(lib, n_fields=3, stride=2) == E.RG_EINVAL and b"stride=2" in lib.rg_last_error()
    assert _grid(lib, n_fields=5, stride=4) == E.RG_EINVAL
    assert _grid(lib, packed=P + 4) == E.RG_EALIGN and b"packed" in lib.rg_last_error()
    assert lib.rg_version() == E.ABI_VERSION == 104                                # no existing signature changed


# ---- 4. the brute-force restatement against the reference's fixtures -----------------------------------------------------
def test_fixtures_are_small_and_complete():
    for w in sc.WEIGHTINGS:
        assert os.path.getsize(os.path.join(GOLDEN, f"g11_section_{w}.npz")) < 1_000_000
        meta, arrays = sc.fixture(w)
        assert meta["weighting"] == w and meta["digest"] == sc.volume().digest()
        assert meta["volume"] == sc.VOLUME and meta["nz"] == sc.NZ and meta["toa"] == sc.TOA
        for name, (vertices, spacing) in sc.PATHS.items():
            xs, ys, s = sc.path_points(name)
            np.testing.assert_array_equal(arrays[f"{name}_xs"], xs)
            np.testing.assert_array_equal(arrays[f"{name}_ys"], ys)
            np.testing.assert_array_equal(arrays[f"{name}_s"], s)
            lengths = np.diff(arrays[f"{name}_indptr"].astype(np.int64))
            assert len(lengths) == sc.NZ * len(xs)
            assert 0.0 < (lengths == 0).mean() <= 0.5
            for f in sc.FIELDS:
                assert {f"{name}_grid_{f}", f"{name}_grid_{f}_qc", f"{name}_grid_{f}_qc_fill"} <= set(arrays)
    _, arrays = sc.fixture("barnes2")
    assert np.diff(arrays["dogleg_indptr"].astype(np.int64)).max() > 1000          # the section through the radar


@pytest.mark.parametrize("name", sorted(sc.PATHS))
def test_brute_force_reproduces_the_reference(name):
    """Neighbour sets exactly; weights to <= 1 ulp for Barnes (two exp implementations) and exactly for the others."""
    ip, idx, _, _ = sc.scene_pairs(name)
    for weighting in sc.WEIGHTINGS:
        _, ref = sc.fixture(weighting)
        r_ip, r_idx, r_w = oracle.canonical_rows(ref[f"{name}_indptr"], ref[f"{name}_gate_indices"], ref[f"{name}_weights"])
        np.testing.assert_array_equal(ip, r_ip)
        np.testing.assert_array_equal(idx, r_idx)
        w = sc.scene_weights(name, weighting, exact=False)
        if weighting == "barnes2":
            ulp = np.abs(w.view(np.int32).astype(np.int64) - r_w.view(np.int32).astype(np.int64))
            assert ulp.max(initial=0) <= 1
        else:
            np.testing.assert_array_equal(w, r_w)


@pytest.mark.parametrize("name", sorted(sc.PATHS))
def test_oracle_apply_on_the_brute_force_rows_matches_the_reference_sections(name):
    vol = sc.volume()
    ip, idx, _, _ = sc.scene_pairs(name)
    n = len(sc.path_points(name)[0])
    shape = (sc.NZ, 1, n)
    for weighting in sc.WEIGHTINGS:
        _, ref = sc.fixture(weighting)
        w = sc.scene_weights(name, weighting, exact=False)
        w64 = sc.scene_weights(name, weighting)
        for f in sc.FIELDS:
            data, mask, mask_qc = sc.field_and_masks(vol, f)
            scale = float(np.nanmax(np.abs(data[~mask])))
            assert_same_to_rounding(oracle.csr_apply(ip, idx, w, data, mask, shape), ref[f"{name}_grid_{f}"], scale)
            assert_same_to_rounding(oracle.csr_apply(ip, idx, w, data, mask_qc, shape), ref[f"{name}_grid_{f}_qc"], scale)
            assert_same_to_rounding(oracle.csr_apply(ip, idx, w, data, mask_qc, shape, fill_value=sc.FILL),
                                    ref[f"{name}_grid_{f}_qc_fill"], scale, fill=sc.FILL)
            # the reference's own float32 section lies within the float64 bound every gridding path is held to
            stats = oracle.voxel_stats(ip, idx, w64, data, mask_qc)
            ratio = oracle.bound_ratio(ref[f"{name}_grid_{f}_qc"], stats, oracle.DELTA_CSR[weighting])
            assert ratio.max(initial=0.0) <= 1.0


def test_brute_force_on_scattered_points():
    """Arbitrary points (unsorted, a duplicate, one far outside the gates) against oracle.build_geometry on 1 x 1 grids
    placed at each of them: the restatement does not need a path."""
    vol = sc.volume()
    rng = np.random.default_rng(5)
    xs = np.float32(rng.uniform(-60e3, 60e3, 7))
    ys = np.float32(rng.uniform(-60e3, 60e3, 7))
    xs[3], ys[3] = xs[0], ys[0]
    xs[5], ys[5] = 200e3, 200e3
    zc = sc.levels(nz=5)
    ip, idx, w = sc.brute_section(vol.gate_x, vol.gate_y, vol.gate_z, xs, ys, zc, "cressman")
    assert ip[-1] > 0
    for i in range(len(xs)):
        o_ip, o_idx, o_w = oracle.build_geometry(vol.gate_x, vol.gate_y, vol.gate_z, (5, 1, 1),
                                                 (sc.Z_LIMITS, (float(ys[i]),) * 2, (float(xs[i]),) * 2),
                                                 weighting="cressman", toa=sc.TOA)
        for k in range(5):
            a, b = ip[k * len(xs) + i], ip[k * len(xs) + i + 1]
            np.testing.assert_array_equal(idx[a:b], o_idx[o_ip[k]:o_ip[k + 1]])
            np.testing.assert_array_equal(w[a:b], o_w[o_ip[k]:o_ip[k + 1]])
    assert ip[5 + 1] - ip[5] == 0
