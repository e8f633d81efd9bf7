"""Several radars on one grid, CPU side: the contract pinned against the reference's fixtures (g10_mosaic_*, built by
tests/golden/make_mosaic_golden.py) through the oracle, the reach windows, the argument validation of the Python surface
(which happens before any device is touched) and of rg_roi_grid_mosaic_f32 (every call here fails validation before a
launch)."""
import ctypes
import os
import re

import numpy as np
import pytest

import mosaic_scenes
import radar_processor_amd as rg
from conftest import GOLDEN, REPO, assert_same_to_rounding, load_golden
from mosaic_scenes import concat_rows  # noqa: F401  (shared with tests/test_gpu_mosaic.py)
from oracle import radar_grid_oracle as oracle
from radar_processor_amd import _native, synthetic

WEIGHTINGS = ("barnes2", "cressman", "nearest")
P = 1 << 12                                  # a 16-byte aligned address that is never dereferenced


# ---- shared with tests/test_gpu_mosaic.py ---------------------------------------------------------------------------
def fixture(weighting):
    meta, arrays = load_golden(f"g10_mosaic_{weighting}")
    return meta, arrays


def fixture_volumes(meta):
    vols = []
    for spec, digest in zip(meta["volumes"], meta["digests"]):
        vol = synthetic.make_volume(fields=tuple(meta["fields"]), **spec)
        assert vol.digest() == digest, "synthetic generator drifted from the one the fixture was made with"
        vols.append(vol)
    return vols


def fixture_grid(meta):
    return tuple(meta["grid_shape"]), tuple(tuple(float(v) for v in lim) for lim in meta["grid_limits"])


def fixture_masks(meta, vols, name):
    """Per radar: field values and exclusion mask (the QC filter folded into its radar's mask)."""
    out = []
    for r, vol in enumerate(vols):
        extra = []
        if r == meta["qc_radar"]:
            extra = [oracle.gate_mask("below", np.ma.getdata(vol.fields[meta["qc"][0]]), meta["qc"][1])]
        out.append(oracle.merge_masks(vol.fields[name], extra))
    return out


def oracle_mosaic(vols, origins, shape, limits, weighting, toa, exact_weights=False, min_radius=250.0,
                  beam_factor=0.01746):
    """Per radar oracle CSR on the shifted limits, and their row-wise concatenation."""
    csrs = [oracle.build_geometry(v.gate_x, v.gate_y, v.gate_z, shape, rg.mosaic_limits(limits, o), radar_altitude=0.0,
                                  min_radius=min_radius, beam_factor=beam_factor, weighting=weighting, toa=toa - o[0],
                                  exact_weights=exact_weights)
            for v, o in zip(vols, origins)]
    offsets = np.concatenate([[0], np.cumsum([len(v.gate_x) for v in vols])]).astype(np.int64)
    return csrs, concat_rows(csrs, offsets), offsets


# ---- 1. mosaic_limits --------------------------------------------------------------------------------------------------
def test_mosaic_limits_arithmetic():
    limits = ((0.0, 10000.0), (-25e3, 29e3), (10e3, 80e3))
    assert rg.mosaic_limits(limits, (0, 0, 0)) == limits
    assert rg.mosaic_limits(limits, (800.0, 10e3, 85e3)) == ((-800.0, 9200.0), (-35e3, 19e3), (-75e3, -5e3))
    got = rg.mosaic_limits(((0, 1), (2, 3), (4, 5)), np.array([0.5, 1.0, 1.5]))
    assert got == ((-0.5, 0.5), (1.0, 2.0), (2.5, 3.5)) and all(type(v) is float for lim in got for v in lim)


# ---- 2. the oracle against the reference's fixtures ------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_oracle_rows_match_reference_per_radar(weighting):
    meta, ref = fixture(weighting)
    vols = fixture_volumes(meta)
    shape, limits = fixture_grid(meta)
    csrs, _, _ = oracle_mosaic(vols, meta["origins"], shape, limits, weighting, meta["toa"])
    for r, (ip, idx, w) in enumerate(csrs):
        r_ip, r_idx, r_w = oracle.canonical_rows(ref[f"r{r}_indptr"], ref[f"r{r}_gate_indices"], ref[f"r{r}_weights"])
        np.testing.assert_array_equal(ip, r_ip)
        np.testing.assert_array_equal(idx, r_idx)
        if weighting == "barnes2":
            ulp = np.abs(w.view(np.int32).astype(np.int64) - r_w.view(np.int32).astype(np.int64))
            assert ulp.max(initial=0) <= 1
        else:
            np.testing.assert_array_equal(w, r_w)
    # every voxel class is there: reached by 0, 1, 2 and 3 radars
    reached = np.sum([np.diff(ip) > 0 for ip, _, _ in csrs], axis=0)
    assert set(np.unique(reached).tolist()) == {0, 1, 2, 3}


@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_oracle_mosaic_apply_matches_reference_grids(weighting):
    meta, ref = fixture(weighting)
    vols = fixture_volumes(meta)
    shape, limits = fixture_grid(meta)
    _, (ip, idx, w), _ = oracle_mosaic(vols, meta["origins"], shape, limits, weighting, meta["toa"])
    for name in meta["fields"]:
        parts = fixture_masks(meta, vols, name)
        data = np.concatenate([d for d, _ in parts])
        mask = np.concatenate([m for _, m in parts])
        scale = float(np.nanmax(np.abs(data[~mask])))
        got = oracle.csr_apply(ip, idx, w, data, mask, shape)
        assert_same_to_rounding(got, ref[f"grid_{name}"], scale)
        got = oracle.csr_apply(ip, idx, w, data, mask, shape, fill_value=meta["fill_value"])
        assert_same_to_rounding(got, ref[f"grid_{name}_fill"], scale, fill=meta["fill_value"])


@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_reference_mosaic_within_the_float64_bound(weighting):
    meta, ref = fixture(weighting)
    vols = fixture_volumes(meta)
    shape, limits = fixture_grid(meta)
    _, (ip, idx, w64), _ = oracle_mosaic(vols, meta["origins"], shape, limits, weighting, meta["toa"], exact_weights=True)
    for name in meta["fields"]:
        parts = fixture_masks(meta, vols, name)
        data = np.concatenate([d for d, _ in parts])
        mask = np.concatenate([m for _, m in parts])
        stats = oracle.voxel_stats(ip, idx, w64, data, mask)
        ratio = oracle.bound_ratio(ref[f"grid_{name}"], stats, oracle.DELTA_CSR[weighting])
        assert ratio.max(initial=0.0) <= 1.0


# ---- 3. reach windows ------------------------------------------------------------------------------------------------------
def _rows_outside(ip, shape, window):
    nz, ny, nx = shape
    counts = np.diff(np.asarray(ip, dtype=np.int64)).reshape(nz, ny, nx)
    inside = np.zeros((ny, nx), dtype=bool)
    iy0, iy1, ix0, ix1 = window
    inside[iy0:iy1, ix0:ix1] = True
    return int(counts[:, ~inside].sum()), int(counts[:, inside].sum())


@pytest.mark.parametrize("beam_factor", [0.01746, 0.0, 0.05])
def test_reach_window_holds_every_neighbour(beam_factor):
    meta, _ = fixture("nearest")
    vols = fixture_volumes(meta)
    shape, limits = fixture_grid(meta)
    csrs, _, _ = oracle_mosaic(vols, meta["origins"], shape, limits, "nearest", meta["toa"], beam_factor=beam_factor)
    cut = 0
    for vol, origin, (ip, _, _) in zip(vols, meta["origins"], csrs):
        w = rg.reach_window(vol.gate_x, vol.gate_y, vol.gate_z, shape, limits, origin, 250.0, beam_factor, meta["toa"])
        outside, inside = _rows_outside(ip, shape, w)
        assert outside == 0 and inside > 0
        cut += w[1] - w[0] < shape[1] or w[3] - w[2] < shape[2]
    assert cut >= 1                                                     # a window does cut the grid here


def test_reach_window_of_a_radar_that_misses_the_grid():
    meta, _ = fixture("nearest")
    vol = fixture_volumes(meta)[0]
    shape, limits = fixture_grid(meta)
    far = (0.0, 600e3, -400e3)
    w = rg.reach_window(vol.gate_x, vol.gate_y, vol.gate_z, shape, limits, far, 250.0, 0.01746, meta["toa"])
    assert w == (0, 0, 0, 0)
    ip, _, _ = oracle.build_geometry(vol.gate_x, vol.gate_y, vol.gate_z, shape, rg.mosaic_limits(limits, far), toa=9000.0,
                                     weighting="nearest")
    assert ip[-1] == 0
    # no valid gate at all (toa below every gate) reaches nothing either; a beam factor outside [0, 1): the whole grid
    assert rg.reach_window(vol.gate_x, vol.gate_y, vol.gate_z, shape, limits, (0, 0, 0), toa=-1e6) == (0, 0, 0, 0)
    assert rg.reach_window(vol.gate_x, vol.gate_y, vol.gate_z, shape, limits, far, beam_factor=1.0) == (0, 28, 0, 36)


def test_reach_window_is_padded_and_clipped():
    shape, limits = (2, 11, 11), ((0.0, 1000.0), (-5000.0, 5000.0), (-5000.0, 5000.0))
    g = np.zeros(1, dtype=np.float32)
    # one gate at the grid centre, reach 250 m: the voxel under it plus one voxel each side
    assert rg.reach_window(g, g, g, shape, limits, (0, 0, 0), 250.0, 0.0) == (4, 7, 4, 7)
    # at the corner: clipped to the grid
    assert rg.reach_window(g, g, g, shape, limits, (0, -5000.0, -5000.0), 250.0, 0.0) == (0, 2, 0, 2)


# ---- 4. validation before any device use -------------------------------------------------------------------------------------
def _radar(n=8, origin=(0.0, 0.0, 0.0)):
    z = np.zeros(n, dtype=np.float32)
    return (z, z, z, origin)


def test_validation_of_the_radars(tmp_path):
    shape, limits = (2, 4, 4), ((0, 1000), (0, 3000), (0, 3000))
    with pytest.raises(ValueError, match="at least one radar"):
        rg.compute_mosaic_geometry([], shape, limits, str(tmp_path))
    with pytest.raises(ValueError, match="origin"):
        rg.compute_mosaic_geometry([_radar(origin=(0.0, 1.0))], shape, limits, str(tmp_path))
    with pytest.raises(ValueError, match="origin"):
        rg.MosaicSearch([_radar(), _radar(origin=(0.0, np.nan, 1.0))], shape, limits)
    with pytest.raises(ValueError, match="gate_x, gate_y and gate_z differ"):
        z = np.zeros(8, dtype=np.float32)
        rg.compute_mosaic_geometry([_radar(), (z, z, z[:7], (0, 0, 0))], shape, limits, str(tmp_path))
    with pytest.raises(ValueError, match=r"\(gate_x, gate_y, gate_z, origin\)"):
        rg.MosaicSearch([_radar()[:3]], shape, limits)
    with pytest.raises(ValueError, match="RG_MAX_RADARS"):
        rg.MosaicSearch([_radar()] * (_native.RG_MAX_RADARS + 1), shape, limits)
    with pytest.raises(ValueError, match="Unknown weighting"):
        rg.compute_mosaic_geometry([_radar()], shape, limits, str(tmp_path), weighting="closest")
    with pytest.raises(ValueError, match="temp_dir"):
        rg.compute_mosaic_geometry([_radar()], shape, limits, str(tmp_path / "missing"))


def test_gate_count_limit_of_both_routes(tmp_path):
    shape, limits = (2, 4, 4), ((0, 1000), (0, 3000), (0, 3000))
    big = np.broadcast_to(np.float32(0.0), (2 ** 30,))         # no memory behind it: only the length is read
    radars = [(big, big, big, (0, 0, 0))] * 2
    with pytest.raises(ValueError, match="2\\^31"):
        rg.MosaicSearch(radars, shape, limits)
    with pytest.raises(ValueError, match="2\\^31"):
        rg.compute_mosaic_geometry(radars, shape, limits, str(tmp_path))


def _host_mosaic_geometry(counts, shape=(1, 2, 2)):
    n_vox = int(np.prod(shape))
    g = rg.GridGeometry(shape, ((0, 1), (0, 1), (0, 1)), np.zeros(n_vox + 1, dtype=np.int32), np.zeros(0, dtype=np.int32),
                        np.zeros(0, dtype=np.float32), 17000.0)
    g.gate_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    g.origins = np.zeros((len(counts), 3))
    return g


def test_validation_of_fields_and_masks():
    torch = pytest.importorskip("torch")
    geom = _host_mosaic_geometry([5, 7])
    f5, f7 = torch.zeros(5), torch.zeros(7)
    with pytest.raises(ValueError, match="fields of 2 radars"):
        rg.mosaic_fields_device(geom, [[f5]])
    with pytest.raises(ValueError, match="radar 1 field 0: 5 values for 7 gates"):
        rg.mosaic_fields_device(geom, [[f5], [f5]])
    with pytest.raises(ValueError, match="radar 1: 2 fields"):
        rg.mosaic_fields_device(geom, [[f5], [f7, f7]])
    with pytest.raises(ValueError, match="one entry \\(tensor or None\\) per field"):
        rg.mosaic_fields_device(geom, [[f5], [f7]], masks=[[None], []])
    with pytest.raises(ValueError, match="radar 0 mask 0: 7 values for 5 gates"):
        rg.mosaic_fields_device(geom, [[f5], [f7]], masks=[[torch.zeros(7, dtype=torch.uint8)], [None]])
    with pytest.raises(ValueError, match="radar 1 mask 1: 5 values"):
        rg.mosaic_fields_device(geom, [[f5], [f7]], shared_masks=[None, torch.zeros(5, dtype=torch.uint8)])
    with pytest.raises(ValueError, match="one entry per radar"):
        rg.mosaic_fields_device(geom, [[f5], [f7]], shared_masks=[None])
    with pytest.raises(ValueError, match="all of its radars"):
        rg.mosaic_fields_device(geom, [[f5]], radars=[0])
    with pytest.raises(ValueError, match="no fields"):
        rg.mosaic_fields_device(geom, [[], []])
    with pytest.raises(ValueError, match="not a mosaic"):
        rg.mosaic_fields_device(_host_mosaic_geometry([5]).__class__((1, 1, 1), None, None, None, None, 0.0), [[f5]])
    with pytest.raises(TypeError):
        rg.mosaic_fields_device(object(), [[f5]])
    with pytest.raises(ValueError, match="one field per radar"):
        rg.apply_mosaic(geom, [np.zeros(5, dtype=np.float32)])
    with pytest.raises(ValueError, match="radar 1 has 7 gates"):
        rg.apply_mosaic(geom, [np.zeros(5, dtype=np.float32), np.zeros(5, dtype=np.float32)])
    with pytest.raises(ValueError, match="one filter list per radar"):
        rg.apply_mosaic(geom, [np.zeros(5, dtype=np.float32), np.zeros(7, dtype=np.float32)], additional_filters=[[]])
    with pytest.raises(ValueError, match="radar 0 has 5 gates"):
        rg.apply_mosaic_multi(geom, {"A": [np.zeros(4, dtype=np.float32), np.zeros(7, dtype=np.float32)]})


def test_gather_limit_of_the_geometry_route():
    torch = pytest.importorskip("torch")
    n = 2 ** 29
    geom = _host_mosaic_geometry([n, n])                    # 2^30 gates: 4 GiB with one packed float per gate
    big = torch.zeros(1).expand(n)                          # no memory behind it
    with pytest.raises(ValueError, match="4 GiB"):
        rg.mosaic_fields_device(geom, [[big], [big]])
    geom = _host_mosaic_geometry([n // 4, n // 4])          # 2^28 gates: fine for one field, not for three (stride 4)
    small = torch.zeros(1).expand(n // 4)
    with pytest.raises(ValueError, match="4 GiB"):
        rg.mosaic_fields_device(geom, [[small] * 3, [small] * 3])
    with pytest.raises(ValueError, match="4 GiB"):
        rg.apply_mosaic_multi(geom, {k: [np.broadcast_to(np.float32(0), (n // 4,))] * 2 for k in "ABC"})


# ---- 5. the C ABI ------------------------------------------------------------------------------------------------------------
def test_mosaic_radar_layout_matches_the_header():
    header = open(os.path.join(REPO, "include", "radargrid_hip.h")).read()
    assert re.search(r"#define RG_MAX_RADARS (\d+)", header).group(1) == str(_native.RG_MAX_RADARS) == "16"
    body = re.search(r"typedef struct rg_mosaic_radar \{(.*?)\} rg_mosaic_radar;", header, re.S).group(1)
    names = re.findall(r"\*?\s*(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [n for n, _ in _native.MosaicRadar._fields_]
    R = _native.MosaicRadar
    assert ctypes.sizeof(_native.CellGrid) == 64
    assert ctypes.sizeof(R) == 136                  # 64-bit pointers, a 64-byte rg_cellgrid, int32 quadruple, two int64
    assert [getattr(R, n).offset for n, _ in R._fields_] == [0, 8, 16, 80, 88, 96, 104, 108, 112, 116, 120, 128]


def _entry(**kw):
    e = _native.MosaicRadar(sorted_gates=P, cell_start=P, xc=P, yc=P, zc=P, ix0=0, iy0=0, nx_win=4, ny_win=4,
                            gate_offset=0, n_gates=10)
    e.cells = _native.CellGrid(x0=0.0, y0=0.0, inv_cx=1e-3, inv_cy=1e-3, z_lo=-1e3, z_hi=1e4, ncx=4, ncy=4, levels=0,
                               level0=0)
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def _mosaic(table, n_radars=None, shape=(2, 4, 4), weighting=0, packed=P, n_fields=1, stride=1, n_total=10):
    lib = rg.load_library(require_device=False)
    arr = None
    if table is not None:
        arr = (_native.MosaicRadar * len(table))(*table)
        n_radars = len(table) if n_radars is None else n_radars
    return lib.rg_roi_grid_mosaic_f32(arr, n_radars or 0, *shape, 250.0, 0.01746, weighting, packed, n_fields, stride,
                                      n_total, 0.0, P, None)


def test_mosaic_entry_point_argument_validation():
    lib = rg.load_library(require_device=False)
    bad = _entry(n_gates=11)                     # every call below also carries an entry the checks refuse: no launch
    assert _mosaic(None, 1) == _native.RG_EINVAL and b"null radar table" in lib.rg_last_error()
    assert _mosaic([bad], n_radars=0) == _native.RG_EINVAL
    assert _mosaic([_entry()] * (_native.RG_MAX_RADARS + 1)) == _native.RG_EUNSUPPORTED
    assert _mosaic([bad], shape=(0, 4, 4)) == _native.RG_EINVAL and b"bad grid shape" in lib.rg_last_error()
    assert _mosaic([bad], shape=(2, 4, 0)) == _native.RG_EINVAL
    assert _mosaic([bad], stride=2) == _native.RG_EINVAL and b"stride=2" in lib.rg_last_error()
    assert _mosaic([bad], n_fields=3, stride=2) == _native.RG_EINVAL
    assert _mosaic([bad], n_fields=9, stride=8) == _native.RG_EUNSUPPORTED
    assert _mosaic([bad], weighting=_native.WEIGHTINGS["closest"]) == _native.RG_EUNSUPPORTED
    assert _mosaic([bad], weighting=7) == _native.RG_EINVAL
    assert _mosaic([bad], packed=P + 4) == _native.RG_EALIGN
    assert _mosaic([bad], packed=None) == _native.RG_EINVAL
    assert _mosaic([bad], n_total=2 ** 31) == _native.RG_EUNSUPPORTED
    # the gate range of every entry must lie inside the packed fields
    assert _mosaic([bad]) == _native.RG_EINVAL and b"exceed n_gates_total" in lib.rg_last_error()
    assert _mosaic([_entry(), _entry(gate_offset=5, n_gates=6)]) == _native.RG_EINVAL
    assert _mosaic([_entry(gate_offset=-1, n_gates=1), bad]) == _native.RG_EINVAL
    # the window must lie inside the grid (checked for entries that reach nothing too)
    for kw in (dict(ix0=1), dict(iy0=2, ny_win=3), dict(ix0=-1, nx_win=1), dict(nx_win=-1), dict(ix0=5, nx_win=0)):
        assert _mosaic([_entry(**kw), bad]) == _native.RG_EINVAL and b"outside the" in lib.rg_last_error(), kw
    # an entry that reaches something needs its search structure
    assert _mosaic([_entry(xc=0), bad]) == _native.RG_EINVAL and b"null pointer" in lib.rg_last_error()
    assert _mosaic([_entry(sorted_gates=P + 8), bad]) == _native.RG_EALIGN
    # ... an entry that reaches nothing does not: its pointers are never read
    assert _mosaic([_entry(nx_win=0, sorted_gates=0, cell_start=0, xc=0), bad]) == _native.RG_EINVAL
    assert b"exceed n_gates_total" in lib.rg_last_error()


def test_validation_of_the_last_slot_of_a_full_table():
    """A 16-entry table (RG_MAX_RADARS) whose slot 15 alone is refused -- its window outside the grid, or its gates past
    n_gates_total: the call fails before any launch and names radar 15 (the checks run over every slot, the last one
    included)."""
    lib = rg.load_library(require_device=False)
    assert _native.RG_MAX_RADARS == 16
    good = [_entry(gate_offset=k % 3, n_gates=7) for k in range(15)]
    for last, what in ((_entry(ix0=1), b"outside the"), (_entry(iy0=3, ny_win=2), b"outside the"),
                       (_entry(gate_offset=5, n_gates=6), b"exceed n_gates_total"),
                       (_entry(nx_win=0, gate_offset=9, n_gates=2, sorted_gates=0, xc=0), b"exceed n_gates_total")):
        assert _mosaic(good + [last]) == _native.RG_EINVAL
        msg = lib.rg_last_error()
        assert b"radar 15:" in msg and what in msg, msg


# ---- 6. many radars: the seeded scenes of tests/mosaic_scenes.py --------------------------------------------------------
@pytest.mark.parametrize("name", ["scene16", "scene20"])
def test_many_radar_scene_properties(name):
    """The scenes exercise what they are built for (mosaic_scenes.check_properties): 16 / 20 radars, a voxel reached by
    >= 8 of them, >= 100 oracle pairs from every live radar, window left edges on >= 8 residues mod 16 and all 4 mod 4,
    every grid face touched, inert radars at slots 0 and 7 and a live one at slot 15, a radar reaching levels below its
    antenna and one whose gates cross its toa - oz cut."""
    scene = getattr(mosaic_scenes, name)()
    assert scene.n_radars == {"scene16": 16, "scene20": 20}[name]
    assert scene.shape[1] % 4 and scene.shape[2] % 16                  # ragged against the 16 x 4 patch
    got = mosaic_scenes.check_properties(scene)
    print(name, got)


@pytest.mark.parametrize("name", ["scene16", "scene20"])
def test_reach_window_is_conservative_on_the_scenes(name):
    """No voxel with an oracle neighbour of radar r lies outside radar r's reach window; an empty window means no pairs."""
    scene = getattr(mosaic_scenes, name)()
    for r in range(scene.n_radars):
        w = scene.window(r)
        ip = scene.csr(r)[0]
        if w == (0, 0, 0, 0):
            assert ip[-1] == 0, r
            continue
        outside, inside = _rows_outside(ip, scene.shape, w)
        assert outside == 0, (r, w, outside)


def _extra_placements():
    """Seeded placements around the scene grid: just outside each face (x, y, below the bottom), antennas above the grid
    top and above toa, for beam factors 0.01746, 0 and 0.05 and minimum radii 250 and 1500."""
    rng = np.random.default_rng(77)
    (z0, z1), (y0, y1), (x0, x1) = mosaic_scenes.LIMITS
    out = []
    for k in range(10):
        d = float(rng.uniform(2e3, 12e3))
        oy, ox = float(rng.uniform(y0, y1)), float(rng.uniform(x0, x1))
        oz = float(rng.uniform(0.0, 3000.0))
        origin = [(oz, oy, x0 - d), (oz, oy, x1 + d), (oz, y0 - d, ox), (oz, y1 + d, ox), (z0 - d / 4, oy, ox),
                  (z1 + d / 10, oy, ox), (mosaic_scenes.TOA + d / 10, oy, ox), (oz, y1 + d, x0 - d), (oz, oy, ox),
                  (oz, y0 - d, x1 + d)][k]
        bf = (0.01746, 0.0, 0.05)[k % 3]
        mr = (250.0, 1500.0)[k % 2]
        spec = mosaic_scenes.RadarSpec(seed=300 + k, max_range_m=float(rng.uniform(18e3, 28e3)), origin=origin)
        out.append((spec, bf, mr))
    return out


def test_reach_window_is_conservative_for_extra_placements():
    shape, limits, toa = mosaic_scenes.SHAPE, mosaic_scenes.LIMITS, mosaic_scenes.TOA
    n_empty = n_cut = 0
    for spec, bf, mr in _extra_placements():
        v = mosaic_scenes.volume(spec)
        w = rg.reach_window(v.gate_x, v.gate_y, v.gate_z, shape, limits, spec.origin, mr, bf, toa)
        ip, _, _ = oracle.build_geometry(v.gate_x, v.gate_y, v.gate_z, shape, rg.mosaic_limits(limits, spec.origin),
                                         min_radius=mr, beam_factor=bf, weighting="nearest", toa=toa - spec.origin[0])
        if w == (0, 0, 0, 0):
            assert ip[-1] == 0, (spec, bf, mr)
            n_empty += 1
            continue
        outside, inside = _rows_outside(ip, shape, w)
        assert outside == 0, (spec, bf, mr, w, outside)
        n_cut += inside > 0 and (w[1] - w[0] < shape[1] or w[3] - w[2] < shape[2])
        # a beam factor outside [0, 1): the whole grid
        for bad in (1.0, -0.01, 2.5):
            assert rg.reach_window(v.gate_x, v.gate_y, v.gate_z, shape, limits, spec.origin, mr, bad, toa) == \
                (0, shape[1], 0, shape[2])
    assert n_empty >= 2 and n_cut >= 5, (n_empty, n_cut)


def test_fixtures_are_small_and_complete():
    for w in WEIGHTINGS:
        path = os.path.join(GOLDEN, f"g10_mosaic_{w}.npz")
        assert os.path.getsize(path) < 1 << 20
        meta, arrays = fixture(w)
        assert meta["weighting"] == w and len(meta["origins"]) == 3 and meta["toa"] == 9000.0
        for r in range(3):
            assert {f"r{r}_indptr", f"r{r}_gate_indices", f"r{r}_weights"} <= set(arrays)
        assert {"grid_DBZH", "grid_RHOHV", "grid_DBZH_fill", "grid_RHOHV_fill"} <= set(arrays)
