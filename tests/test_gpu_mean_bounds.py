"""Every gridding path held to the per-voxel error bound of oracle.mean_error_bound, and K2's weights observed directly.

 1. On every reference fixture with neighbours (g2 / g3 / g4 / g6), each path's grid against the float64 mean of its
    voxel (exact weights, oracle.voxel_stats): NaN pattern equal, and ``|got - m| <= bound`` with the path's delta
    (oracle.DELTA_CSR: the CSR paths multiply with the reference's float32 weights; oracle.DELTA_K2: the CSR-free gridder
    computes its own).  Paths: ``apply_geometry`` (K1), the row-wise packed kernel in a 1-field pass and in an 8-field pass
    (one weight-sum chain, oracle.ROWWISE_WEIGHT_CHAINS), and K2 (``rg_roi_grid_f32``) with every RoiSearch variant of
    test_gpu_roi_rim for 1 field and for 3 fields with a shared QC mask.  The worst err / bound per path and fixture is
    printed as one JSON line and, where the environment names a report directory (RG_REPORT_DIR), written to
    mean_bounds.json in it.
 2. K2 weight probes: voxels far apart against their ROI, each with exactly two live neighbours -- a gate at the voxel
    centre (d2f = 0: its weight is exactly the float32 ``1 + 1e-5`` / 1 / 1) valued 0 and a gate at d2 / r2 = q valued
    1 -- so the gridded value ``w2 / (w1 + w2)`` gives the kernel's weight ratio to a few u.  q covers [0, 1) and the
    2e-6 rim band, near the radar (min_radius ROI) and at 240 km (beam ROI, coordinates of 2.4e5), for all three
    weightings; the recovered relative weight error must stay within the budget rg_roi_grid.hip states plus 8u.
"""
import functools
import json
import os

import numpy as np
import pytest

from conftest import builder_kwargs, golden_names, grid_spec, load_golden, reference_indices, volume_for
from oracle import radar_grid_oracle as oracle
from oracle import roi_rim

pytestmark = pytest.mark.gpu

FIXTURES = [n for n in golden_names("g2_") + golden_names("g3_") + golden_names("g4_") + golden_names("g6_")
            if n != "g3_c2_corner_barnes2"]                     # the corner window has no neighbours
SEARCHES = (dict(), dict(per_level=False), dict(per_level=True, cell_size=1.0), dict(per_level=False, cell_size=1.0))
REPORT = {}


@pytest.fixture(scope="module")
def rg():
    import radar_processor_amd as pkg
    pkg.load_library()
    return pkg


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    print("mean_bounds", json.dumps(REPORT, sort_keys=True))
    out_dir = os.environ.get("RG_REPORT_DIR")
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "mean_bounds.json"), "w") as fh:
            json.dump(REPORT, fh, indent=1, sort_keys=True)


@functools.lru_cache(maxsize=2)
def _fixture(name):
    meta, ref = load_golden(name)
    vol = volume_for(meta)
    shape, limits = grid_spec(meta)
    kw = builder_kwargs(meta)
    weighting = kw.pop("weighting")
    kw.pop("toa")
    idx = reference_indices(name, meta, ref)
    w64 = oracle.pair_weights_f64(ref["indptr"], idx, vol.gate_x, vol.gate_y, vol.gate_z, shape, limits, weighting=weighting,
                                  **kw)
    qc_field, qc_min = meta["qc"] if "qc" in meta else (meta["fields"][0], 10.0)   # single-field fixtures: a mask of their own
    qc = oracle.gate_mask("below", np.ma.getdata(vol.fields[qc_field]), qc_min)
    return meta, ref, vol, idx, w64, (qc, qc_field, qc_min)


def _check(name, path, got, stats, delta):
    """Assert the bound on every voxel of ``got`` and record the worst err / bound of (path, fixture)."""
    r = oracle.bound_ratio(got, stats, delta)
    worst = float(r.max(initial=0.0))
    rec = REPORT.setdefault(path, {})
    rec[name] = max(rec.get(name, 0.0), worst)
    assert worst <= 1.0, (path, name, worst, int((r > 1).sum()))


# ---- 1. every path, every fixture ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_every_path_within_the_bound(rg, name):
    import torch
    from radar_processor_amd.gridding import CsrGridder
    dev = torch.device("cuda", 0)
    meta, ref, vol, idx, w64, (qc, qc_field, qc_min) = _fixture(name)
    shape, limits = grid_spec(meta)
    weighting = meta["weighting"]
    names = list(meta["fields"])
    ip = ref["indptr"]
    d_csr, d_k2 = oracle.DELTA_CSR[weighting], oracle.DELTA_K2[weighting]
    plain = [oracle.merge_masks(vol.fields[f]) for f in names]
    with_qc = [(d, m | qc) for d, m in plain]
    stats = {(i, q): oracle.voxel_stats(ip, idx, w64, *(with_qc if q else plain)[i]) for i in range(len(names)) for q in (0, 1)}
    to_dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=dt)

    # K1: apply_geometry on the reference's CSR
    geom = rg.GridGeometry(shape, limits, ip, idx, ref["weights"], toa=meta["toa"])
    radar = vol.as_radar()
    gf = rg.GateFilter(radar).exclude_below(qc_field, qc_min)
    assert int(gf.n_excluded()) == int(qc.sum())
    for i, f in enumerate(names):
        fdata = rg.get_field_data(radar, f)
        _check(name, "k1", rg.apply_geometry(geom, fdata), stats[i, 0], d_csr)
        _check(name, "k1", rg.apply_geometry(geom, fdata, additional_filters=[gf]), stats[i, 1], d_csr)

    # row-wise kernel over the packed records: 1 field (two weight chains) and 8 fields (one chain)
    if weighting != "cressman":                                 # Cressman weights reach 0: no 26-bit code
        compact = geom.device_compact(dev)
        for label, group in (("rowwise_1f", [(0, 0)]), ("rowwise_1f", [(0, 1)]),
                             ("rowwise_8f", [(k % len(names), k % 2) for k in range(8)])):
            gr = CsrGridder(geom, vol.n_total_gates, len(group), device=dev)
            gr.compact, gr.window = compact, compact.window_for(len(group))
            gr.packed_stream = compact.ensure_packed(gr.csr)
            assert gr.packed_stream
            src = [(with_qc if q else plain)[i] for i, q in group]
            gr.pack([to_dev(d, torch.float32) for d, _ in src], [to_dev(m, torch.uint8) for _, m in src])
            out = torch.empty((len(group), gr.n_vox), dtype=torch.float32, device=dev)
            gr.apply(out)
            got = out.cpu().numpy()
            for k, (i, q) in enumerate(group):
                _check(name, label, got[k], stats[i, q], d_csr)

    # K2: every RoiSearch variant, 1 field, and 3 fields with a shared QC mask
    kw = builder_kwargs(meta)
    kw.pop("weighting")
    f_t = [to_dev(d, torch.float32) for d, _ in plain]
    m_t = [to_dev(m, torch.uint8) for _, m in plain]
    three = [k % len(names) for k in range(3)]
    qc_t = to_dev(qc, torch.uint8)
    for skw in SEARCHES:
        search = rg.RoiSearch(vol.gate_x, vol.gate_y, vol.gate_z, shape, limits, device=dev, **kw, **skw)
        label = "k2" + "".join(f"_{k}={v}" for k, v in skw.items())
        got = rg.roi_grid_fields_device(search, f_t[:1], m_t[:1], weighting=weighting).cpu().numpy()
        _check(name, label + "_1f", got[0], stats[0, 0], d_k2)
        got = rg.roi_grid_fields_device(search, [f_t[i] for i in three], [m_t[i] for i in three], shared_mask=qc_t,
                                        weighting=weighting).cpu().numpy()
        for k, i in enumerate(three):
            _check(name, label + "_3f_qc", got[k], stats[i, 1], d_k2)


# ---- 2. K2 weight probes ----------------------------------------------------------------------------------------------
# Voxel spacing > 2 r_max in every direction: a gate within r of its voxel is farther than r from every other voxel.
PROBE_GRIDS = {
    # min_radius ROI (250 m) near the radar, 2 km spacing
    "near": dict(shape=(2, 9, 9), limits=((500.0, 3500.0), (-8e3, 8e3), (-8e3, 8e3)), min_radius=250.0, beam_factor=0.01746),
    # beam ROI at 240 km (0.01746 * |v| ~ 4.2 km), 12 km spacing, float32 coordinates of 2.4e5
    "far": dict(shape=(1, 6, 6), limits=((2000.0, 2000.0), (-30e3, 30e3), (225e3, 285e3)), min_radius=250.0,
                beam_factor=0.01746),
}
Q_TARGETS = tuple(np.linspace(0.0, 0.995, 28)) + ("band",) * 8    # d2 / r2 of the probe gate; 'band': in the 2e-6 rim band


def _probe_cloud(grid, seed):
    """Per voxel: gate 0 at the centre (value 0), gate 1 at d2 / r2 = q (value 1), gate 2 anywhere inside (masked, value
    1e4).  Returns gx, gy, gz, values, mask, q_of_voxel (actual d2 / r2 of gate 1)."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = grid["shape"]
    zc, yc, xc = roi_rim.voxel_centres(grid["shape"], grid["limits"])
    pts, val, msk, q_of = [], [], [], []
    for v in range(nz * ny * nx):
        iz, rem = divmod(v, ny * nx)
        iy, ix = divmod(rem, nx)
        rim = roi_rim.voxel_rim(xc[ix], yc[iy], zc[iz], grid["min_radius"], grid["beam_factor"])
        c = np.array([rim.x, rim.y, rim.z])
        target = Q_TARGETS[v % len(Q_TARGETS)]
        if target == "band":
            g1 = roi_rim.plant(rim, "B", rng)
            assert g1 is not None
        else:
            u = rng.normal(size=3)
            u /= np.linalg.norm(u)
            g1 = (c + u * np.sqrt(target * rim.r2)).astype(np.float32)
        u = rng.normal(size=3)
        g2 = (c + u / np.linalg.norm(u) * np.sqrt(0.5 * rim.r2)).astype(np.float32)
        pts += [c.astype(np.float32), g1, g2]
        val += [0.0, 1.0, 1e4]
        msk += [False, False, True]
        q_of.append(float(roi_rim.d2_f64(g1[0:1], g1[1:2], g1[2:3], rim.x, rim.y, rim.z)[0] / rim.r2))
    p = np.array(pts, dtype=np.float32)
    return p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy(), np.array(val, np.float32), np.array(msk), np.array(q_of)


@pytest.mark.parametrize("weighting", ("barnes2", "cressman", "nearest"))
def test_k2_weight_probes(rg, weighting):
    import torch
    dev = torch.device("cuda", 0)
    budget = oracle.K2_WEIGHT_BUDGET[weighting]
    worst, probes, q_all = 0.0, 0, []
    for gname, grid in sorted(PROBE_GRIDS.items()):
        gx, gy, gz, val, msk, q = _probe_cloud(grid, seed=len(gname))
        shape, limits = grid["shape"], grid["limits"]
        kw = dict(min_radius=grid["min_radius"], beam_factor=grid["beam_factor"])
        ip, idx, w64 = oracle.build_geometry(gx, gy, gz, shape, limits, weighting=weighting, exact_weights=True, **kw)
        n_vox = int(np.prod(shape))
        # exactly gates 3v, 3v + 1, 3v + 2 are the neighbours of voxel v, in that order
        np.testing.assert_array_equal(np.diff(ip), np.full(n_vox, 3))
        np.testing.assert_array_equal(idx, np.arange(3 * n_vox))
        assert np.all(q < 1.0)
        exact_ratio = w64[1::3] / w64[0::3]
        f_t = torch.from_numpy(val).to(dev)
        m_t = torch.from_numpy(msk.astype(np.uint8)).to(dev)
        for skw in SEARCHES[:2]:
            search = rg.RoiSearch(gx, gy, gz, shape, limits, device=dev, **kw, **skw)
            m = rg.roi_grid_fields_device(search, [f_t], [m_t], weighting=weighting)[0].cpu().numpy().ravel().astype(np.float64)
            assert np.all(np.isfinite(m)) and np.all((m > 0) & (m < 1)), (gname, skw)
            ratio = m / (1.0 - m)                                  # w2 / w1 as the kernel weighed them
            rel = np.abs(ratio / exact_ratio - 1.0)
            k = int(np.argmax(rel))
            print(f"{weighting} {gname} {skw}: worst recovered weight error {rel[k]:.3g} ({rel[k] / oracle.U32:.1f} u) "
                  f"at d2/r2 = {q[k]:.7f}")
            worst = max(worst, float(rel.max()))
            probes += n_vox
        q_all.append(q)
    q_all = np.concatenate(q_all)
    REPORT.setdefault("k2_weight_probes", {})[weighting] = dict(max_rel_weight_error=worst, probes=probes, budget=budget)
    # coverage: the whole range of d2 / r2, the rim band, both ROI regimes (2 grids x 2 searches x their voxels)
    assert probes == 2 * (2 * 9 * 9 + 6 * 6)
    for lo, hi in ((0.0, 1e-12), (1e-12, 0.25), (0.25, 0.5), (0.5, 0.75), (0.75, 0.99), (0.99, 1 - 2e-6)):
        assert np.count_nonzero((q_all >= lo) & (q_all < hi)) >= 3, (lo, hi)
    assert np.count_nonzero(q_all >= 1 - 2.5e-6) >= 8
    assert worst <= budget + 8 * oracle.U32, (weighting, worst)
