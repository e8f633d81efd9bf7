"""Several radars on one grid, on the MI355X: the mosaic geometry and both gridding routes against the reference's
fixtures (g10_mosaic_*), the float64 mosaic mean and the single-radar paths they reduce to."""
import ctypes

import numpy as np
import pytest

from conftest import assert_same_to_rounding
from test_mosaic_host import WEIGHTINGS, concat_rows, fixture, fixture_grid, fixture_masks, fixture_volumes, oracle_mosaic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native
    rg.load_library()
    return dict(torch=torch, rg=rg, native=_native, dev=torch.device("cuda", 0))


def _radars(vols, origins):
    return [(v.gate_x, v.gate_y, v.gate_z, tuple(o)) for v, o in zip(vols, origins)]


def _dev(env, a, dtype=None):
    torch = env["torch"]
    return torch.from_numpy(np.ascontiguousarray(a)).to(env["dev"], dtype=dtype or torch.float32)


def _ulp(a, b):
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64)
                  - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


def _radar_of_pairs(ip, idx, offsets):
    """Radar of every pair and row of every pair, asserting the row layout: radar 0's pairs, then radar 1's, ..."""
    ip = np.asarray(ip, dtype=np.int64)
    radar = np.searchsorted(np.asarray(offsets), np.asarray(idx, dtype=np.int64), side="right") - 1
    row = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    assert np.all((np.diff(radar) >= 0) | (np.diff(row) > 0)), "a row is not radar 0's pairs, then radar 1's, ..."
    return radar, row


def _segments(ip, idx, w, offsets, r):
    """Radar r's segment of every mosaic row, as a CSR over the radar's own gate numbers."""
    radar, row = _radar_of_pairs(ip, idx, offsets)
    keep = radar == r
    counts = np.bincount(row[keep], minlength=len(ip) - 1)
    return (np.concatenate([[0], np.cumsum(counts)]), (np.asarray(idx, dtype=np.int64)[keep] - offsets[r]).astype(np.int32),
            np.asarray(w)[keep])


def _rows(ip, idx, w, rows):
    """Sub-CSR of whole rows ``rows`` (in that order)."""
    lengths = ip[rows + 1] - ip[rows]
    take = np.concatenate([np.arange(ip[v], ip[v + 1]) for v in rows])
    return np.concatenate([[0], np.cumsum(lengths)]), np.asarray(idx)[take], np.asarray(w)[take]


def _geometry(env, meta, vols, weighting, tmp_path):
    shape, limits = fixture_grid(meta)
    return env["rg"].compute_mosaic_geometry(_radars(vols, meta["origins"]), shape, limits, str(tmp_path),
                                             weighting=weighting, toa=meta["toa"])


# ---- 1. the mosaic geometry ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_mosaic_geometry_matches_reference(env, weighting, tmp_path):
    import oracle.radar_grid_oracle as oracle
    meta, ref = fixture(weighting)
    vols = fixture_volumes(meta)
    shape, limits = fixture_grid(meta)
    geom = _geometry(env, meta, vols, weighting, tmp_path)
    offsets = np.concatenate([[0], np.cumsum([len(v.gate_x) for v in vols])])
    np.testing.assert_array_equal(geom.gate_offsets, offsets)
    assert geom.gate_offsets.dtype == np.int64 and geom.origins.shape == (3, 3) and geom.origins.dtype == np.float64
    assert geom.grid_limits == limits and geom.toa == meta["toa"]
    ref_csrs = [(ref[f"r{r}_indptr"], ref[f"r{r}_gate_indices"], ref[f"r{r}_weights"]) for r in range(3)]
    np.testing.assert_array_equal(np.asarray(geom.indptr, dtype=np.int64), concat_rows(ref_csrs, offsets)[0])
    for r in range(3):
        ip, idx, w = oracle.canonical_rows(*_segments(geom.indptr, geom.gate_indices, geom.weights, offsets, r))
        r_ip, r_idx, r_w = oracle.canonical_rows(*ref_csrs[r])
        np.testing.assert_array_equal(ip, r_ip)
        np.testing.assert_array_equal(idx, r_idx)
        if weighting == "barnes2":
            assert _ulp(w, r_w).max(initial=0) <= 1
        else:
            np.testing.assert_array_equal(w, r_w)


# ---- 2. apply_mosaic / apply_mosaic_multi against the reference's mosaic grids -----------------------------------------------
def _assert_relative(got, want, scale, rtol=1e-5):
    sig = np.isfinite(want) & (np.abs(want) >= 0.05 * scale)
    assert sig.sum() > 50
    rel = np.abs(got[sig].astype(np.float64) - want[sig]) / np.abs(want[sig].astype(np.float64))
    assert rel.max() <= rtol


@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_apply_mosaic_matches_reference_grids(env, weighting, tmp_path):
    rg, torch = env["rg"], env["torch"]
    meta, ref = fixture(weighting)
    vols = fixture_volumes(meta)
    shape, _ = fixture_grid(meta)
    geom = _geometry(env, meta, vols, weighting, tmp_path)
    radars = [v.as_radar() for v in vols]
    qc = [[rg.GateFilter(radars[r]).exclude_below(*meta["qc"])] if r == meta["qc_radar"] else [] for r in range(3)]
    fields = {name: [rg.get_field_data(rad, name) for rad in radars] for name in meta["fields"]}
    multi = rg.apply_mosaic_multi(geom, fields, {name: qc for name in fields}, fill_value=meta["fill_value"])
    for name in meta["fields"]:
        parts = fixture_masks(meta, vols, name)
        data = np.concatenate([d for d, _ in parts])
        mask = np.concatenate([m for _, m in parts])
        scale = float(np.nanmax(np.abs(data[~mask])))
        got = rg.apply_mosaic(geom, fields[name], qc)
        assert got.dtype == np.float32 and got.shape == shape
        assert_same_to_rounding(got, ref[f"grid_{name}"], scale)
        _assert_relative(got, ref[f"grid_{name}"], scale)
        assert_same_to_rounding(multi[name], ref[f"grid_{name}_fill"], scale, fill=meta["fill_value"])
        _assert_relative(multi[name], ref[f"grid_{name}_fill"], scale)
        # the device route: the same pass, the same bits
        dev_grid = rg.mosaic_fields_device(geom, [[_dev(env, d)] for d, _ in parts],
                                           masks=[[_dev(env, m.astype(np.uint8), torch.uint8)] for _, m in parts],
                                           fill_value=meta["fill_value"])
        np.testing.assert_array_equal(dev_grid[0].cpu().numpy().view(np.int32), multi[name].view(np.int32))


# ---- 3. identity: one radar at the origin IS compute_grid_geometry ----------------------------------------------------------
@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_one_radar_at_origin_is_compute_grid_geometry(env, weighting, tmp_path):
    rg = env["rg"]
    meta, _ = fixture(weighting)
    vol = fixture_volumes(meta)[0]
    shape, limits = fixture_grid(meta)
    assert rg.reach_window(vol.gate_x, vol.gate_y, vol.gate_z, shape, limits, (0, 0, 0), toa=meta["toa"]) == (0, 28, 0, 36)
    mos = rg.compute_mosaic_geometry([(vol.gate_x, vol.gate_y, vol.gate_z, (0.0, 0.0, 0.0))], shape, limits, str(tmp_path),
                                     weighting=weighting, toa=meta["toa"])
    one = rg.compute_grid_geometry(vol.gate_x, vol.gate_y, vol.gate_z, shape, limits, str(tmp_path), weighting=weighting,
                                   toa=meta["toa"])
    for k in ("indptr", "gate_indices", "weights"):
        a, b = getattr(mos, k), getattr(one, k)
        assert a.dtype == b.dtype and a.shape == b.shape
        np.testing.assert_array_equal(a.view(np.int32) if a.dtype == np.float32 else a,
                                      b.view(np.int32) if b.dtype == np.float32 else b)
    radar = vol.as_radar()
    gf = rg.GateFilter(radar).exclude_below("RHOHV", 0.8)
    f = rg.get_field_data(radar, "DBZH")
    got = rg.apply_mosaic(mos, [f], [[gf]], fill_value=-1.0)
    want = rg.apply_geometry(one, f, [gf], fill_value=-1.0)
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))


# ---- 4. windowing changes nothing -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", ["barnes2", "cressman"])
def test_windowed_segments_equal_whole_grid_builds(env, weighting, tmp_path):
    """Each radar's segment of the mosaic equals, bit for bit and in the same in-row order, compute_grid_geometry on the
    shifted limits over the whole grid: a windowed search bins its gates on the whole grid's cell lattice."""
    rg = env["rg"]
    meta, _ = fixture(weighting)
    vols = fixture_volumes(meta)
    shape, limits = fixture_grid(meta)
    geom = _geometry(env, meta, vols, weighting, tmp_path)
    windows = [rg.reach_window(v.gate_x, v.gate_y, v.gate_z, shape, limits, o, toa=meta["toa"])
               for v, o in zip(vols, meta["origins"])]
    assert any(w != (0, shape[1], 0, shape[2]) for w in windows)
    for r, (vol, o) in enumerate(zip(vols, meta["origins"])):
        one = rg.compute_grid_geometry(vol.gate_x, vol.gate_y, vol.gate_z, shape, rg.mosaic_limits(limits, o), str(tmp_path),
                                       weighting=weighting, toa=meta["toa"] - o[0])
        seg = _segments(geom.indptr, geom.gate_indices, geom.weights, geom.gate_offsets, r)
        np.testing.assert_array_equal(seg[0], np.asarray(one.indptr, dtype=np.int64))
        np.testing.assert_array_equal(seg[1], one.gate_indices)
        np.testing.assert_array_equal(seg[2].view(np.int32), one.weights.view(np.int32))


@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_one_radar_narrower_than_the_grid_is_compute_grid_geometry(env, weighting, tmp_path):
    """One radar at the origin of a grid wider than its reach: its window is a part of the grid, and the mosaic still IS
    compute_grid_geometry -- the same arrays bit for bit (in-row order included) and the same grids from apply_mosaic."""
    rg, torch = env["rg"], env["torch"]
    meta, _ = fixture(weighting)
    vol = fixture_volumes(meta)[2]
    shape, limits = (6, 40, 56), ((0.0, 10000.0), (-130e3, 104e3), (-150e3, 125e3))
    w = rg.reach_window(vol.gate_x, vol.gate_y, vol.gate_z, shape, limits, (0, 0, 0), toa=meta["toa"])
    assert 0 < w[1] - w[0] < shape[1] and 0 < w[3] - w[2] < shape[2]
    gx, gy, gz = (torch.from_numpy(a).to(env["dev"]) for a in (vol.gate_x, vol.gate_y, vol.gate_z))   # device-resident
    mos = rg.compute_mosaic_geometry([(gx, gy, gz, (0.0, 0.0, 0.0))], shape, limits, str(tmp_path), weighting=weighting,
                                     toa=meta["toa"])
    one = rg.compute_grid_geometry(vol.gate_x, vol.gate_y, vol.gate_z, shape, limits, str(tmp_path), weighting=weighting,
                                   toa=meta["toa"])
    assert one.n_pairs() > 0
    # the window's search bins on the whole grid's cell lattice, cropped to the window
    sw = rg.RoiSearch(vol.gate_x, vol.gate_y, vol.gate_z, shape, limits, toa=meta["toa"], window=w)
    sf = rg.RoiSearch(vol.gate_x, vol.gate_y, vol.gate_z, shape, limits, toa=meta["toa"])
    assert sw.cells.inv_cx == sf.cells.inv_cx and sw.cells.ncx < sf.cells.ncx and sw.cells.ncy < sf.cells.ncy
    kx, ky = (sw.cells.x0 - sf.cells.x0) * sf.cells.inv_cx, (sw.cells.y0 - sf.cells.y0) * sf.cells.inv_cy
    assert abs(kx - round(kx)) < 1e-6 and abs(ky - round(ky)) < 1e-6
    for k in ("indptr", "gate_indices", "weights"):
        a, b = getattr(mos, k), getattr(one, k)
        assert a.dtype == b.dtype and a.shape == b.shape
        np.testing.assert_array_equal(a.view(np.int32) if a.dtype == np.float32 else a,
                                      b.view(np.int32) if b.dtype == np.float32 else b)
    radar = vol.as_radar()
    gf = rg.GateFilter(radar).exclude_below("RHOHV", 0.8)
    f = rg.get_field_data(radar, "DBZH")
    np.testing.assert_array_equal(rg.apply_mosaic(mos, [f], [[gf]]).view(np.int32),
                                  rg.apply_geometry(one, f, [gf]).view(np.int32))


# ---- 6. K2 identity: one table entry is rg_roi_grid_f32 ---------------------------------------------------------------------
def _entry_of(native, s, offset=0):
    e = native.MosaicRadar(sorted_gates=native.ptr(s.sorted_gates), cell_start=native.ptr(s.cell_start),
                           xc=native.ptr(s.xc), yc=native.ptr(s.yc), zc=native.ptr(s.zc), gate_offset=offset,
                           n_gates=s.n_gates)
    e.cells = s.cells
    iy0, iy1, ix0, ix1 = s.window
    e.ix0, e.iy0, e.nx_win, e.ny_win = ix0, iy0, ix1 - ix0, iy1 - iy0
    return e


@pytest.mark.parametrize("per_level", [True, False])
@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_one_entry_returns_the_bits_of_rg_roi_grid(env, weighting, per_level):
    torch, rg, native = env["torch"], env["rg"], env["native"]
    meta, _ = fixture(weighting)
    vol = fixture_volumes(meta)[1]
    shape, limits = fixture_grid(meta)
    lim = rg.mosaic_limits(limits, meta["origins"][1])
    s = rg.RoiSearch(vol.gate_x, vol.gate_y, vol.gate_z, shape, lim, toa=meta["toa"] - meta["origins"][1][0],
                     per_level=per_level)
    assert s.per_level == per_level and s.window == (0, shape[1], 0, shape[2])
    lib = native.load_library()
    n = s.n_gates
    nz, ny, nx = shape
    gen = torch.Generator(device="cpu").manual_seed(5)
    for nf in (1, 2, 3, 8):
        stride = 1 if nf == 1 else 2 if nf == 2 else 4 if nf <= 4 else 8
        vals = [(torch.rand(n, generator=gen) * 70 - 10).to(env["dev"]) for _ in range(nf)]
        masks = [(torch.rand(n, generator=gen) < 0.3).to(torch.uint8).to(env["dev"]) for _ in range(nf)]
        packed = torch.empty(n * stride, dtype=torch.float32, device=env["dev"])
        fp = (ctypes.c_void_p * nf)(*[native.ptr(v) for v in vals])
        mp = (ctypes.c_void_p * nf)(*[native.ptr(m) for m in masks])
        native.check(lib.rg_pack_fields_f32(nf, fp, mp, None, n, stride, native.ptr(packed), native.stream_ptr()), "pack")
        a = torch.empty((nf, nz * ny * nx), dtype=torch.float32, device=env["dev"])
        b = torch.empty_like(a)
        native.check(lib.rg_roi_grid_f32(native.ptr(s.sorted_gates), native.ptr(s.cell_start), s.cells, native.ptr(s.xc),
                                         native.ptr(s.yc), native.ptr(s.zc), nz, ny, nx, s.min_radius, s.beam_factor,
                                         native.WEIGHTINGS[weighting], native.ptr(packed), nf, stride, float("nan"),
                                         native.ptr(a), native.stream_ptr()), "rg_roi_grid_f32")
        table = (native.MosaicRadar * 1)(_entry_of(native, s))
        native.check(lib.rg_roi_grid_mosaic_f32(table, 1, nz, ny, nx, s.min_radius, s.beam_factor,
                                                native.WEIGHTINGS[weighting], native.ptr(packed), nf, stride, n,
                                                float("nan"), native.ptr(b), native.stream_ptr()), "rg_roi_grid_mosaic_f32")
        assert torch.isfinite(a).any()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{nf} fields"


# ---- 7. MosaicSearch against the float64 mosaic mean ---------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_mosaic_search_within_the_float64_bound(env, weighting):
    rg, torch = env["rg"], env["torch"]
    import oracle.radar_grid_oracle as oracle
    meta, ref = fixture(weighting)
    vols = fixture_volumes(meta)
    shape, limits = fixture_grid(meta)
    ms = rg.MosaicSearch(_radars(vols, meta["origins"]), shape, limits, toa=meta["toa"])
    _, (ip, idx, w64), _ = oracle_mosaic(vols, meta["origins"], shape, limits, weighting, meta["toa"], exact_weights=True)
    parts = {n: fixture_masks(meta, vols, n) for n in meta["fields"]}
    # 2 fields: the value ring; 3 and 8: the strides 4 and 8, which gather per hit at each radar's gate offset
    for names in (list(meta["fields"]), ["DBZH", "RHOHV", "DBZH"], ["DBZH", "RHOHV"] * 4):
        fields = [[_dev(env, parts[n][r][0]) for n in names] for r in range(3)]
        masks = [[_dev(env, parts[n][r][1].astype(np.uint8), torch.uint8) for n in names] for r in range(3)]
        got = rg.mosaic_fields_device(ms, fields, masks=masks, weighting=weighting)
        assert got.shape[0] == len(names)
        for k, n in enumerate(names):
            data = np.concatenate([d for d, _ in parts[n]])
            mask = np.concatenate([m for _, m in parts[n]])
            stats = oracle.voxel_stats(ip, idx, w64, data, mask)
            assert oracle.bound_ratio(got[k].cpu().numpy(), stats, oracle.DELTA_K2[weighting]).max(initial=0.0) <= 1.0
            assert_same_to_rounding(got[k], ref[f"grid_{n}"], float(np.nanmax(np.abs(data[~mask]))))


def test_mosaic_search_products_are_the_planes_of_its_grid(env):
    """The CSR-free route with a PlaneProducts: the planes column_argmax / column_min / column_mean / constant_altitude_ppi
    give on the grid the same call returns without products, bit for bit."""
    rg, torch = env["rg"], env["torch"]
    meta, _ = fixture("barnes2")
    vols = fixture_volumes(meta)
    shape, limits = fixture_grid(meta)
    ms = rg.MosaicSearch(_radars(vols, meta["origins"]), shape, limits, toa=meta["toa"])
    fields = [[_dev(env, np.ma.getdata(v.fields[n])) for n in ("DBZH", "RHOHV")] for v in vols]
    shared = [_dev(env, np.ma.getmaskarray(v.fields["DBZH"]).astype(np.uint8), torch.uint8) for v in vols]
    spec = rg.PlaneProducts(colmax=True, argmax=True, colmin=True, colmean=True, cappi=(3000.0, 4000.0, 99000.0))
    recs = rg.mosaic_fields_device(ms, fields, shared_masks=shared, products=spec)
    grids = rg.mosaic_fields_device(ms, fields, shared_masks=shared)
    assert len(recs) == 2
    bits = lambda t: t.contiguous().view(torch.int32)
    for k, rec in enumerate(recs):
        cmax, carg = rg.column_argmax(grids[k])
        assert torch.equal(bits(rec["colmax"]), bits(cmax)) and torch.equal(rec["argmax"], carg)
        assert torch.equal(bits(rec["colmin"]), bits(rg.column_min(grids[k])))
        assert torch.equal(bits(rec["colmean"]), bits(rg.column_mean(grids[k])))
        for alt in (3000.0, 4000.0, 99000.0):
            assert torch.equal(bits(rec["cappi"][alt]), bits(rg.constant_altitude_ppi(grids[k], ms, alt))), alt


# ---- 8. subsets and inert radars -----------------------------------------------------------------------------------------------
def test_subsets_and_inert_radars(env):
    rg, torch = env["rg"], env["torch"]
    import oracle.radar_grid_oracle as oracle
    from radar_processor_amd import synthetic
    meta, _ = fixture("barnes2")
    vols = fixture_volumes(meta)
    shape, limits = fixture_grid(meta)
    origins = [tuple(o) for o in meta["origins"]]
    # inert: far away (empty window), and a small radar inside the grid whose gates sit halfway between two levels
    far = vols[0]
    tiny = synthetic.make_volume(n_elev=1, n_az=36, n_gates=20, seed=3, fields=("DBZH", "RHOHV"), max_range_m=3000.0)
    tiny.gate_z = np.full_like(tiny.gate_z, 1000.0)
    o_far, o_tiny = (0.0, 900e3, 0.0), (0.0, 0.0, 40e3)
    assert rg.reach_window(far.gate_x, far.gate_y, far.gate_z, shape, limits, o_far, toa=meta["toa"]) == (0, 0, 0, 0)
    assert rg.reach_window(tiny.gate_x, tiny.gate_y, tiny.gate_z, shape, limits, o_tiny, toa=meta["toa"]) != (0, 0, 0, 0)
    all_vols = vols[:1] + [far, tiny] + vols[1:]
    all_origins = origins[:1] + [o_far, o_tiny] + origins[1:]
    ms = rg.MosaicSearch(_radars(all_vols, all_origins), shape, limits, toa=meta["toa"])
    assert ms.searches[1] is None and ms.searches[2] is not None and ms.searches[2].count_pairs() == 0
    names = ["DBZH", "RHOHV"]
    fields = [[_dev(env, np.ma.getdata(v.fields[n])) for n in names] for v in all_vols]
    shared = [np.ma.getmaskarray(v.fields["DBZH"]).astype(np.uint8) for v in all_vols]
    shared_t = [_dev(env, m, torch.uint8) for m in shared]
    base = rg.mosaic_fields_device(ms, [fields[0], fields[3], fields[4]], shared_masks=[shared_t[0], shared_t[3], shared_t[4]],
                                   radars=[0, 3, 4])
    with_inert = rg.mosaic_fields_device(ms, fields, shared_masks=shared_t)
    assert torch.equal(base.view(torch.int32), with_inert.view(torch.int32))
    # radars 0 and 2 of the three: within the bound of the float64 mean of those two
    sub = rg.mosaic_fields_device(ms, [fields[0], fields[4]], shared_masks=[shared_t[0], shared_t[4]], radars=[0, 4])
    pair = [vols[0], vols[2]]
    _, (ip, idx, w64), _ = oracle_mosaic(pair, [origins[0], origins[2]], shape, limits, "barnes2", meta["toa"],
                                         exact_weights=True)
    mask = np.concatenate([shared[0], shared[4]]).astype(bool)
    for k, n in enumerate(names):
        data = np.concatenate([np.ma.getdata(v.fields[n]) for v in pair])
        stats = oracle.voxel_stats(ip, idx, w64, data, mask)
        assert oracle.bound_ratio(sub[k].cpu().numpy(), stats, oracle.DELTA_K2["barnes2"]).max(initial=0.0) <= 1.0
    assert not torch.equal(sub.view(torch.int32), base.view(torch.int32))


# ---- 5. full size: three C2 radars, the compact pass, K1, products ------------------------------------------------------------
FULL_SHAPE = (6, 500, 200)                                          # 480 m columns, as the C2 grid: 78 M pairs
FULL_LIMITS = ((0.0, 15e3), (-120e3, 119.52e3), (-48e3, 47.52e3))
FULL_ORIGINS = [(0.0, -60e3, -100e3), (500.0, 20e3, 110e3), (200.0, 150e3, 0.0)]


@pytest.fixture(scope="module")
def full(env, tmp_path_factory):
    rg = env["rg"]
    from radar_processor_amd import synthetic
    cfg = synthetic.CONFIGS["C2"]
    vols = [synthetic.make_volume(cfg["n_elev"], cfg["n_az"], cfg["n_gates"], seed=40 + r, fields=("DBZH", "RHOHV"))
            for r in range(3)]
    radars = _radars(vols, FULL_ORIGINS)
    geom = rg.compute_mosaic_geometry(radars, FULL_SHAPE, FULL_LIMITS, str(tmp_path_factory.mktemp("mosaic")))
    return dict(vols=vols, radars=radars, geom=geom)


def test_full_size_mosaic(env, full):
    rg, torch, dev = env["rg"], env["torch"], env["dev"]
    import oracle.radar_grid_oracle as oracle
    from radar_processor_amd import gridding
    from radar_processor_amd.gridding import CsrGridder
    geom, vols = full["geom"], full["vols"]
    csr = geom.device_csr(dev)
    assert csr.n_pairs >= 50_000_000
    ip = np.asarray(geom.indptr, dtype=np.int64)
    radar, row = _radar_of_pairs(ip, geom.gate_indices, geom.gate_offsets)
    reached = np.zeros(csr.n_vox, dtype=np.int64)
    for r in range(3):
        reached += np.bincount(row[radar == r], minlength=csr.n_vox) > 0
    assert reached.max() == 3
    del radar, row
    assert gridding._use_compact(geom, dev)
    per_pass = gridding.fields_per_pass(geom, dev)
    names = ["DBZH", "RHOHV"] * (per_pass // 2)
    fields = [[_dev(env, np.ma.getdata(v.fields[n])) for n in names] for v in vols]
    shared = [_dev(env, np.ma.getmaskarray(v.fields["DBZH"]).astype(np.uint8), torch.uint8) for v in vols]
    got = rg.mosaic_fields_device(geom, fields, shared_masks=shared)
    assert got.shape[0] == per_pass
    # a one-field pass streams the packed records of the compact copy; a chunk of the mosaic holds the gates of three radars,
    # so wider passes may exceed the copy's LDS window and stay on the standard kernel (CsrGridder's existing policy)
    one = [fs[:1] for fs in fields]
    got1 = rg.mosaic_fields_device(geom, one, shared_masks=shared)
    gr = gridding._cached_gridder(geom, int(geom.gate_offsets[-1]), 1, dev, compact=True)
    assert gr.compact is not None and gr.packed_stream
    assert_same_to_rounding(got1[0], got[0], float(np.nanmax(np.abs(np.ma.getdata(vols[0].fields["DBZH"])))))
    # against K1 (rg_csr_apply_f32 over the plain CSR) and the oracle on sampled whole rows
    cat = [torch.cat([fields[r][f] for r in range(3)]) for f in range(per_pass)]
    cat_m = torch.cat(shared)
    mask = cat_m.cpu().numpy().astype(bool)
    k1 = CsrGridder(geom, cat[0].numel(), per_pass, device=dev, compact=False)
    assert k1.compact is None
    k1.pack(cat, None, cat_m)
    want = torch.empty((per_pass, csr.n_vox), dtype=torch.float32, device=dev)
    k1.apply(want)
    rows = np.random.default_rng(0).choice(csr.n_vox, 20000, replace=False)
    sub_ip, sub_idx, sub_w = _rows(ip, geom.gate_indices, geom.weights, rows)
    for f in range(per_pass):
        data = cat[f].cpu().numpy()
        scale = float(np.nanmax(np.abs(data[~mask])))
        assert_same_to_rounding(got[f].view(-1), want[f], scale)
        o = oracle.csr_apply(sub_ip, sub_idx, sub_w, data, mask, (len(rows),))
        assert_same_to_rounding(got[f].view(-1)[torch.from_numpy(rows).to(dev)], o, scale)
    # products: the fused epilogue's planes equal the separate kernels on the stored mosaic grid
    kw = dict(colmax=True, argmax=True, cappi=(2500.0,), colmin=True, colmean=True)
    fused = rg.mosaic_fields_device(geom, one, shared_masks=shared, products=rg.PlaneProducts(fused=True, **kw))
    sep = rg.mosaic_fields_device(geom, one, shared_masks=shared, products=rg.PlaneProducts(fused=False, **kw))
    grid = rg.mosaic_fields_device(geom, one, shared_masks=shared)[0]
    assert torch.equal(grid.view(torch.int32), got1[0].view(torch.int32))
    for key in ("colmax", "argmax", "colmin", "colmean"):
        assert torch.equal(fused[0][key].view(torch.int32), sep[0][key].view(torch.int32)), key
    assert torch.equal(fused[0]["cappi"][2500.0].view(torch.int32), sep[0]["cappi"][2500.0].view(torch.int32))
    assert torch.equal(sep[0]["colmax"].view(torch.int32), rg.column_max(grid).view(torch.int32))


def test_full_size_mosaic_search_within_the_bound(env, full):
    rg, torch = env["rg"], env["torch"]
    import oracle.radar_grid_oracle as oracle
    geom, vols = full["geom"], full["vols"]
    ms = rg.MosaicSearch(full["radars"], FULL_SHAPE, FULL_LIMITS)
    fields = [[_dev(env, np.ma.getdata(v.fields["DBZH"]))] for v in vols]
    shared = [_dev(env, np.ma.getmaskarray(v.fields["DBZH"]).astype(np.uint8), torch.uint8) for v in vols]
    got = rg.mosaic_fields_device(ms, fields, shared_masks=shared)[0].view(-1)
    # float64 mean on sampled whole rows of the mosaic geometry (the same neighbour sets), weights recomputed per radar
    n_vox = int(np.prod(FULL_SHAPE))
    rows = np.sort(np.random.default_rng(1).choice(n_vox, 20000, replace=False))
    ip = np.asarray(geom.indptr, dtype=np.int64)
    idx = np.asarray(geom.gate_indices, dtype=np.int64)
    offsets = np.asarray(geom.gate_offsets)
    keep_row = np.zeros(n_vox, dtype=bool)
    keep_row[rows] = True
    row_of = np.repeat(np.arange(n_vox), np.diff(ip))
    sel = keep_row[row_of]
    w64 = np.zeros(len(idx), dtype=np.float64)
    for r, (vol, o) in enumerate(zip(vols, FULL_ORIGINS)):
        pr = sel & (idx >= offsets[r]) & (idx < offsets[r + 1])
        counts = np.bincount(row_of[pr], minlength=n_vox)
        sub_ip = np.concatenate([[0], np.cumsum(counts)])
        w64[pr] = oracle.pair_weights_f64(sub_ip, idx[pr] - offsets[r], vol.gate_x, vol.gate_y, vol.gate_z, FULL_SHAPE,
                                          rg.mosaic_limits(FULL_LIMITS, o), weighting="barnes2")
    sub_ip, sub_idx, sub_w = _rows(ip, idx, w64, rows)
    data = np.concatenate([np.ma.getdata(v.fields["DBZH"]) for v in vols])
    mask = np.concatenate([np.ma.getmaskarray(v.fields["DBZH"]) for v in vols])
    stats = oracle.voxel_stats(sub_ip, sub_idx, sub_w, data, mask)
    g = got[torch.from_numpy(rows).to(env["dev"])].cpu().numpy()
    assert oracle.bound_ratio(g, stats, oracle.DELTA_K2["barnes2"]).max(initial=0.0) <= 1.0
