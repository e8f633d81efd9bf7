"""The planes mode of the row-wise kernel (rg_csr_compact_apply_planes_f32, csrc/rg_csr_columns.hip) and the two halves of the
constant-elevation PPI around it (rg_elevation_ppi_plan_f32 / rg_elevation_ppi_finish_f32, csrc/rg_products.hip):

 * against the REFERENCE's product fixtures, bit for bit, with no 3-D grid ever stored: column minimum / mean over all levels and
   over an altitude window (g5, radar_grid/products.py:493-580) for 1-4 fused fields, and every constant-elevation PPI of g7
   (products.py:168-314: five angles, linear / nearest, curved / flat earth, ke = 1), several angles per launch and more than
   one launch holds;
 * against the separate kernels (rg_column_reduce_f32 / rg_elevation_ppi_f32) applied to the row-wise kernel's grid from the
   same gridder, bit for bit -- on the reference's CSRs, on random hand-made CSRs and at full size (config 2), for 1-4 fields,
   1-3 level pieces, index and altitude windows, with and without the 3-D store (which must equal
   rg_csr_compact_apply_packed_f32's grid);
 * through VolumeBatch.grid_shard(products=PlaneProducts(...)) on the CSR route and on the CSR-free (RoiSearch) route.
"""
import numpy as np
import pytest

from conftest import golden_names, load_golden, reference_indices

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rg():
    import radar_processor_amd as pkg
    pkg.load_library()
    return pkg


def _same_bits(a, b):
    import torch
    a, b = a.contiguous(), b.contiguous()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    view = torch.int64 if a.element_size() == 8 else torch.int32
    return torch.equal(a.view(view), b.view(view))


def _gridder(geom, compact, n_gates, nf, dev):
    from radar_processor_amd.gridding import CsrGridder
    g = CsrGridder(geom, n_gates, nf, device=dev)
    g.compact, g.window, g.packed_stream = compact, compact.window_for(nf), True
    assert g.has_columns_kernel
    return g


def _count_planes_launches(monkeypatch):
    from radar_processor_amd.gridding import CsrGridder
    calls = []
    orig = CsrGridder.apply_planes

    def spy(self, *a, **kw):
        calls.append(len(kw.get("sel_levels", ())))
        return orig(self, *a, **kw)
    monkeypatch.setattr(CsrGridder, "apply_planes", spy)
    return calls


def _identity_geometry(rg, grid, limits, **kw):
    """Voxel v's only neighbour is gate v with weight 1.0: the gridding returns the fixture's own values ((1.0 * v) / 1.0 == v;
    NaN voxels are masked gates), so products-only passes must reproduce the reference's planes bit for bit."""
    import torch
    n = grid.size
    geom = rg.GridGeometry(grid.shape, limits, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32),
                           np.ones(n, dtype=np.float32), toa=17000.0, **kw)
    dev = torch.device("cuda", 0)
    compact = geom.device_compact(dev)                 # cached: grid_products_device then runs through the packed records
    assert compact is not None and compact.ensure_packed(geom.device_csr(dev))
    flat = grid.reshape(-1)
    f_t = torch.from_numpy(np.nan_to_num(flat, nan=123.0)).to(dev)
    m_t = torch.from_numpy(np.isnan(flat).astype(np.uint8)).to(dev)
    return geom, f_t, m_t


@pytest.mark.parametrize("name", golden_names("g5_"))
def test_fused_column_min_mean_bit_for_bit_with_the_reference_fixtures(rg, name, monkeypatch):
    meta, ref = load_golden(name)
    grid = ref["grid"]
    geom, f_t, m_t = _identity_geometry(rg, grid, (tuple(meta["z_limits"]), (-1e4, 1e4), (-1.4e4, 1.4e4)))
    import torch
    calls = _count_planes_launches(monkeypatch)
    eq = np.testing.assert_array_equal
    for nf in range(1, 5):
        before = len(calls)
        recs = rg.grid_products_device(geom, [f_t] * nf, [m_t] * nf, fused=True,
                                       products=rg.PlaneProducts(colmin=True, colmean=True, cappi=(4000.0,)))
        assert len(recs) == nf and calls[before:] == [0]                      # one planes-mode launch for the group
        for rec in recs:
            assert rec["colmin"].dtype == rec["colmean"].dtype == torch.float32
            eq(rec["colmin"].cpu().numpy(), ref["P_colmin"])
            eq(rec["colmean"].cpu().numpy(), ref["P_colmean"])
            eq(rec["colmax"].cpu().numpy(), ref["P_colmax"])                    # the column mode's products are unchanged
            eq(rec["cappi"][4000.0].cpu().numpy(), ref["P_cappi4000_linear"])
        alt = rg.grid_products_device(geom, [f_t] * nf, [m_t] * nf, fused=True,
                                      products=rg.PlaneProducts(colmax=False, argmax=False, colmean=True, z_min_alt=1000,
                                                                z_max_alt=8000))
        for rec in alt:
            assert sorted(rec) == ["colmean"]
            eq(rec["colmean"].cpu().numpy(), ref["P_colmean_alt"])
    # the separate route of the same request: the same planes
    plain = rg.grid_products_device(geom, [f_t], [m_t], products=rg.PlaneProducts(colmin=True, colmean=True), fused=False)[0]
    eq(plain["colmin"].cpu().numpy(), ref["P_colmin"])
    eq(plain["colmean"].cpu().numpy(), ref["P_colmean"])


def test_fused_elevation_ppi_bit_for_bit_with_the_reference_fixtures(rg, monkeypatch):
    meta, ref = load_golden("g7_ppi")
    grid = ref["grid"]
    limits = tuple(tuple(float(x) for x in v) for v in meta["grid_limits"])
    geom, f_t, m_t = _identity_geometry(rg, grid, limits, radar_altitude=meta["radar_altitude"])
    calls = _count_planes_launches(monkeypatch)
    keys = sorted(k for k in ref if k.startswith("ppi_e") and not k.endswith("_ke1"))
    assert len(keys) == 20
    combos = sorted({tuple(k.split("_")[2:]) for k in keys})
    angles = sorted({float(k.split("_")[1][1:]) for k in keys})
    assert len(angles) == 5                            # more than RG_MAX_SEL_PLANES: the host splits them over two launches
    n = 0
    for interp, curv in combos:
        for nf in (1, 2):
            before = len(calls)
            recs = rg.grid_products_device(geom, [f_t] * nf, [m_t] * nf, fused=True,
                                           products=rg.PlaneProducts(colmax=False, argmax=False, ppi=angles,
                                                                     ppi_interpolation=interp,
                                                                     earth_curvature=(curv == "curved")))
            assert calls[before:] == [4, 1]
            for rec in recs:
                assert sorted(rec) == ["ppi"] and sorted(rec["ppi"]) == angles
                for e in angles:
                    want = ref[f"ppi_e{e}_{interp}_{curv}"]
                    got = rec["ppi"][e].cpu().numpy()
                    assert got.dtype == want.dtype, (e, interp, curv)
                    np.testing.assert_array_equal(got, want, err_msg=f"{e} {interp} {curv}")
            n += 1
    assert n == 8
    rec = rg.grid_products_device(geom, [f_t], [m_t], fused=True,
                                  products=rg.PlaneProducts(colmax=False, argmax=False, ppi=(2.0, 0.5), ke=1.0))[0]
    np.testing.assert_array_equal(rec["ppi"][2.0].cpu().numpy(), ref["ppi_e2.0_linear_ke1"])
    assert calls[-1] == 2


def _check_against_separate(rg, geom, gridder, row, nf, pieces, window, angles, store):
    """One planes-mode pass against the separate kernels on `row` (the row-wise kernel's grid) -- bit for bit."""
    import torch
    from radar_processor_amd import grid_products as gp
    nz, ny, nx = gridder.grid_shape
    dev = row.device
    lo, hi = window
    full = lambda *s, dt=torch.float32: torch.full(s, -7, dtype=dt, device=dev)
    cmax, carg, cmin = full(nf, ny, nx), full(nf, ny, nx, dt=torch.int32), full(nf, ny, nx)
    mean = pieces == 1
    cmean = full(nf, ny, nx) if mean else None
    out = full(nf, nz * ny * nx) if store else None
    keep_lo, n_keep = (nz // 2, 1)
    planes = full(nf, n_keep, ny, nx)
    plans = [(e, interp, gp.ppi_plan(geom, e, interp, curved, device=dev), curved) for e, interp, curved in angles]
    samples = full(nf, len(plans), 2, ny, nx) if plans else None
    gridder.apply_planes(out=out, level_planes=planes, keep_lo=keep_lo, col_max=cmax, col_arg=carg, col_min=cmin,
                         col_mean=cmean, col_window=(lo, hi), sel_levels=[p[2][0] for p in plans], sel_samples=samples,
                         z_pieces=pieces)
    if store:
        assert _same_bits(out, row), (nf, pieces, window)
    for k in range(nf):
        grid = row[k].view(nz, ny, nx)
        want_max, want_arg = rg.column_argmax(grid, z_min_idx=lo, z_max_idx=hi)
        assert _same_bits(cmax[k], want_max) and torch.equal(carg[k], want_arg), (nf, pieces, window, k)
        assert _same_bits(cmin[k], rg.column_min(grid, z_min_idx=lo, z_max_idx=hi)), (nf, pieces, window, k)
        if mean:
            assert _same_bits(cmean[k], rg.column_mean(grid, z_min_idx=lo, z_max_idx=hi)), (nf, window, k)
        assert _same_bits(planes[k], grid[keep_lo:keep_lo + n_keep])
        for j, (e, interp, plan, curved) in enumerate(plans):
            got = gp.ppi_finish(plan, samples[k, j], interp)
            want = rg.constant_elevation_ppi(grid, geom, e, interpolation=interp, earth_curvature=curved)
            assert _same_bits(got, want), (nf, pieces, e, interp, curved, k)


_ANGLES = [(0.5, "linear", True), (3.0, "nearest", True), (20.0, "linear", False), (60.0, "nearest", False)]


def _paired_c2_fixtures():
    """g3 fixtures whose weights are codable (no Cressman zeros) and that hold pairs at all."""
    return [n for n in golden_names("g3_c2_") if "cressman" not in n and load_golden(n)[1]["weights"].size]


@pytest.mark.parametrize("name", _paired_c2_fixtures())
def test_planes_kernel_on_the_reference_geometries(rg, name):
    import torch
    from oracle import radar_grid_oracle as oracle
    from conftest import volume_for
    from radar_processor_amd.grid_geometry import GridGeometry
    meta, ref = load_golden(name)
    vol = volume_for(meta)
    dev = torch.device("cuda", 0)
    shape = tuple(meta["grid_shape"])
    limits = tuple(tuple(float(x) for x in lim) for lim in meta["grid_limits"])
    gidx = reference_indices(name, meta, ref)
    geom = GridGeometry(shape, limits, ref["indptr"], gidx, ref["weights"], toa=meta["toa"])
    compact = geom.device_compact(dev)
    assert compact is not None and compact.ensure_packed(geom.device_csr(dev))
    names = list(meta["fields"])
    data_mask = [oracle.merge_masks(vol.fields[f]) for f in names]
    f_t = [torch.from_numpy(np.ascontiguousarray(d)).to(dev) for d, _ in data_mask]
    m_t = [torch.from_numpy(m.astype(np.uint8)).to(dev) for _, m in data_mask]
    nz = shape[0]
    for nf in range(1, 5):
        idx = [i % len(names) for i in range(nf)]
        g = _gridder(geom, compact, f_t[0].numel(), nf, dev)
        g.pack([f_t[i] for i in idx], [m_t[i] for i in idx])
        row = torch.empty((nf, g.n_vox), dtype=torch.float32, device=dev)
        g.apply(row)
        for pieces in sorted({1, min(2, nz), min(3, nz)}):
            for window in ((0, nz - 1), (1, nz - 2)):
                _check_against_separate(rg, geom, g, row, nf, pieces, window, _ANGLES, store=(pieces + nf) % 2 == 0)
        _check_against_separate(rg, geom, g, row, nf, 1, (0, nz - 1), [], store=True)
    # altitude windows through the public entry point: fused == separate
    spec = dict(colmin=True, colmean=True, ppi=(1.0, 7.5), z_min_alt=1000.0, z_max_alt=8000.0, cappi=(4000.0,))
    a = rg.grid_products_device(geom, f_t[:3], m_t[:3], products=rg.PlaneProducts(**spec), fused=True)
    b = rg.grid_products_device(geom, f_t[:3], m_t[:3], products=rg.PlaneProducts(**spec), fused=False)
    for ra, rb in zip(a, b):
        assert sorted(ra) == sorted(rb)
        for key in ("colmax", "argmax", "colmin", "colmean"):
            assert _same_bits(ra[key], rb[key]), key
        for e in (1.0, 7.5):
            assert _same_bits(ra["ppi"][e], rb["ppi"][e]), e
        assert _same_bits(ra["cappi"][4000.0], rb["cappi"][4000.0])


@pytest.mark.parametrize("seed", range(6))
def test_planes_kernel_fuzz(rg, seed):
    """Random hand-made CSRs (ragged lines, empty and over-long rows, int32 / int64 row pointers, NaN / Inf values, masks)."""
    import torch
    from radar_processor_amd.grid_geometry import DeviceCSR, GridGeometry
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(9100 + seed)
    nz, ny, nx = int(rng.integers(3, 9)), int(rng.integers(1, 11)), int(rng.integers(1, 200))
    n_vox = nz * ny * nx
    n_gates = int(rng.integers(50, 50_000))
    lengths = rng.integers(0, int(rng.choice([3, 40])), size=n_vox)
    lengths[rng.random(n_vox) < rng.choice([0.0, 0.3])] = 0
    lengths[int(rng.integers(0, n_vox))] = int(rng.integers(400, 1200))
    indptr = np.zeros(n_vox + 1, dtype=np.int64)
    np.cumsum(lengths, out=indptr[1:])
    n_pairs = int(indptr[-1])
    base = rng.integers(0, n_gates, size=n_vox)
    gidx = ((base[np.repeat(np.arange(n_vox), lengths)] + rng.integers(0, 2000, size=n_pairs)) % n_gates).astype(np.int32)
    wts = np.exp(-4.0 * rng.random(n_pairs)).astype(np.float32) + np.float32(1e-5)
    ip_t = torch.from_numpy(indptr if seed % 2 else indptr.astype(np.int32)).to(dev)
    csr = DeviceCSR(ip_t, torch.from_numpy(gidx).to(dev), torch.from_numpy(wts).to(dev), int(gidx.max()))
    limits = ((0.0, float(rng.choice([3000.0, 12000.0]))), (-40e3, 40e3), (-60e3, 60e3))
    geom = GridGeometry.from_device((nz, ny, nx), limits, csr, 17000.0)
    compact = geom.device_compact(dev)
    assert compact is not None and compact.ensure_packed(csr)
    fields = [torch.from_numpy(rng.normal(10, 20, n_gates).astype(np.float32)).to(dev) for _ in range(4)]
    masks = [torch.from_numpy((rng.random(n_gates) < 0.3).astype(np.uint8)).to(dev) if k % 2 == 0 else None
             for k in range(4)]
    fields[1][::7] = float("nan")
    fields[2][3::11] = float("inf")
    for nf in range(1, 5):
        g = _gridder(geom, compact, n_gates, nf, dev)
        g.pack(fields[:nf], masks[:nf])
        row = torch.empty((nf, g.n_vox), dtype=torch.float32, device=dev)
        g.apply(row)
        for pieces in (1, 2, 3):
            _check_against_separate(rg, geom, g, row, nf, pieces, (0, nz - 1), _ANGLES, store=pieces == 2)
        _check_against_separate(rg, geom, g, row, nf, 2, (1, nz - 2), _ANGLES[:2], store=False)


def test_planes_mode_at_size_c2(rg, tmp_path):
    """Config 2 (20 x 1000 x 1000, synthetic.CONFIGS["C2"]): three fields with every product fused against the separate route
    of the same request, bit for bit."""
    import torch
    from radar_processor_amd import synthetic
    cfg = synthetic.CONFIGS["C2"]
    vol = synthetic.make_volume(cfg["n_elev"], cfg["n_az"], cfg["n_gates"], seed=3, fields=("DBZH", "ZDR", "RHOHV"))
    geom = rg.compute_grid_geometry(vol.gate_x, vol.gate_y, vol.gate_z, cfg["grid_shape"], cfg["grid_limits"], str(tmp_path))
    dev = torch.device("cuda", 0)
    compact = geom.device_compact(dev)
    assert compact is not None and compact.ensure_packed(geom.device_csr(dev))
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=dt)
    fields = [to(np.ma.getdata(v), torch.float32) for v in vol.fields.values()]
    masks = [to(np.ma.getmaskarray(v), torch.uint8) for v in vol.fields.values()]
    spec = dict(colmin=True, colmean=True, cappi=(4000.0,), ppi=(0.5, 1.5), z_min_idx=1, z_max_idx=18)
    fused = rg.grid_products_device(geom, fields, masks, products=rg.PlaneProducts(**spec), fused=True)
    plain = rg.grid_products_device(geom, fields, masks, products=rg.PlaneProducts(**spec), fused=False)
    for a, b in zip(fused, plain):
        for key in ("colmax", "argmax", "colmin", "colmean"):
            assert _same_bits(a[key], b[key]), key
        assert _same_bits(a["cappi"][4000.0], b["cappi"][4000.0])
        for e in (0.5, 1.5):
            assert a["ppi"][e].dtype == torch.float64 and _same_bits(a["ppi"][e], b["ppi"][e]), e
        assert bool(torch.isfinite(a["colmean"]).any()) and bool(torch.isfinite(a["ppi"][0.5]).any())


def test_volume_batch_plane_products(rg, tmp_path):
    """Two volumes of two fields: four field-volumes, one pass on every route (fused or not), so the stored grids the planes are
    compared with come from a pass of the same field count -- the same order of float32 adds."""
    import torch
    from radar_processor_amd import batch, synthetic
    dev = torch.device("cuda", 0)
    shape, limits = (6, 20, 70), ((0.0, 6000.0), (-50e3, 50e3), (-60e3, 60e3))
    vols = [synthetic.make_volume(n_elev=4, n_az=90, n_gates=100, seed=40 + b, fields=("DBZH", "ZDR")) for b in range(2)]
    geom = rg.compute_grid_geometry(vols[0].gate_x, vols[0].gate_y, vols[0].gate_z, shape, limits, str(tmp_path))
    compact = geom.device_compact(dev)
    assert compact is not None and compact.ensure_packed(geom.device_csr(dev))
    search = rg.RoiSearch(vols[0].gate_x, vols[0].gate_y, vols[0].gate_z, shape, limits, device=dev)
    volumes = [{k: (np.ma.getdata(v.fields[k]), np.ma.getmaskarray(v.fields[k])) for k in ("DBZH", "ZDR")} for v in vols]
    for geometry in (geom, search):
        vb = batch.VolumeBatch(geometry, ["DBZH", "ZDR"], device=dev)
        assert vb.volumes_per_pass >= 2
        grids = vb.grid_shard(volumes, rank=0, world_size=1)
        for fused in (None, True):
            spec = rg.PlaneProducts(colmin=True, colmean=True, ppi=(0.5,), cappi=(4000.0,), fused=fused)
            recs = vb.grid_shard(volumes, products=spec, rank=0, world_size=1)
            for b in range(2):
                for i in range(2):
                    g, rec = grids[b][i], recs[b][i]
                    assert sorted(rec) == ["argmax", "cappi", "colmax", "colmean", "colmin", "ppi"]
                    want_max, want_arg = rg.column_argmax(g)
                    assert _same_bits(rec["colmax"], want_max) and torch.equal(rec["argmax"], want_arg)
                    assert _same_bits(rec["colmin"], rg.column_min(g))
                    assert _same_bits(rec["colmean"], rg.column_mean(g))
                    assert _same_bits(rec["cappi"][4000.0], rg.constant_altitude_ppi(g, geometry, 4000.0).contiguous())
                    assert _same_bits(rec["ppi"][0.5], rg.constant_elevation_ppi(g, geometry, 0.5))
