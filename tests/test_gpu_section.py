"""Vertical cross-sections on the GPU (csrc/rg_roi_section.hip) against the reference's fixtures g11_section_* and the
per-sample float64 bound.

 1. ``compute_section_geometry`` against the fixture rows after oracle.canonical_rows: counts and index sets equal, weights
    exact for cressman / nearest and <= 1 ulp (fewer than 1e-3 of them differing) for barnes2 -- the rule of
    test_gpu_parity; ``apply_geometry`` and the other consumers of a geometry on it against the fixture's sections.
 2. ``section_fields_device`` held to oracle.mean_error_bound with oracle.DELTA_K2 on every sample (fill pattern equal,
    err / bound <= 1): 1 field, 3 fields with a shared QC mask, 5 fields, every RoiSearch variant of
    test_gpu_mean_bounds.SEARCHES and a windowed search.  The worst ratio per path and weighting is printed as one JSON
    line and written to section_bounds.json where RG_REPORT_DIR names a directory.
 3. Consistency with the lattice (a section along one grid row), independence of the points' order, and
    ``vertical_section`` end to end.
"""
import json
import os

import numpy as np
import pytest

import section_scenes as sc
from conftest import assert_same_to_rounding
from oracle import radar_grid_oracle as oracle
from test_gpu_mean_bounds import SEARCHES

pytestmark = pytest.mark.gpu

PATHS = sorted(sc.PATHS)
REPORT = {}


@pytest.fixture(scope="module")
def rg():
    import radar_processor_amd as pkg
    pkg.load_library()
    return pkg


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    print("section_bounds", json.dumps(REPORT, sort_keys=True))
    out_dir = os.environ.get("RG_REPORT_DIR")
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "section_bounds.json"), "w") as fh:
            json.dump(REPORT, fh, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def scene(rg):
    """The fixture volume on the device: fields, masks, the QC mask, and the default search structure."""
    import torch
    dev = torch.device("cuda", 0)
    vol = sc.volume()
    to_dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=dt)
    host = {f: sc.field_and_masks(vol, f) for f in sc.FIELDS}
    s = dict(vol=vol, dev=dev, host=host,
             f={f: to_dev(host[f][0], torch.float32) for f in sc.FIELDS},
             m={f: to_dev(host[f][1], torch.uint8) for f in sc.FIELDS},
             qc_t=to_dev(oracle.gate_mask("below", np.ma.getdata(vol.fields[sc.QC[0]]), sc.QC[1]), torch.uint8))
    s["search"] = make_search(rg, s)
    return s


def make_search(rg, scene, **kw):
    vol = scene["vol"]
    return rg.RoiSearch(vol.gate_x, vol.gate_y, vol.gate_z, sc.GRID_SHAPE, sc.GRID_LIMITS, toa=sc.TOA,
                        min_radius=sc.MIN_RADIUS, beam_factor=sc.BEAM_FACTOR, device=scene["dev"], **kw)


def stats_of(scene, name, weighting, field, qc):
    ip, idx, _, _ = sc.scene_pairs(name)
    data, mask, mask_qc = scene["host"][field]
    return oracle.voxel_stats(ip, idx, sc.scene_weights(name, weighting), data, mask_qc if qc else mask)


def check_bound(name, weighting, got, stats, what):
    r = oracle.bound_ratio(got, stats, oracle.DELTA_K2[weighting])
    worst = float(r.max(initial=0.0))
    rec = REPORT.setdefault(name, {})
    rec[weighting] = max(rec.get(weighting, 0.0), worst)
    assert worst <= 1.0, (name, weighting, what, worst, int((r > 1).sum()))


# ---- 1. the section as a geometry ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", sc.WEIGHTINGS)
@pytest.mark.parametrize("name", PATHS)
def test_section_geometry_matches_the_reference(rg, scene, name, weighting):
    _, ref = sc.fixture(weighting)
    xs, ys, s = sc.path_points(name)
    geom = rg.compute_section_geometry(scene["search"], xs, ys, weighting)
    assert geom.grid_shape == (sc.NZ, 1, len(xs))
    s_last = float(np.hypot(np.diff(xs.astype(np.float64)), np.diff(ys.astype(np.float64))).sum())
    assert geom.grid_limits == (sc.Z_LIMITS, (0.0, 0.0), (0.0, s_last))
    assert 0.999 * s[-1] < s_last <= s[-1] * (1 + 1e-6)         # point to point: a corner between two samples is cut
    np.testing.assert_array_equal(geom.section_x, xs)
    np.testing.assert_array_equal(geom.section_y, ys)
    assert geom.indptr.dtype == np.int32 and geom.toa == sc.TOA
    ip, idx, w = oracle.canonical_rows(geom.indptr, geom.gate_indices, geom.weights)
    r_ip, r_idx, r_w = oracle.canonical_rows(ref[f"{name}_indptr"], ref[f"{name}_gate_indices"], ref[f"{name}_weights"])
    np.testing.assert_array_equal(ip, r_ip)
    np.testing.assert_array_equal(idx, r_idx)
    if weighting == "barnes2":
        ulp = np.abs(w.view(np.int32).astype(np.int64) - r_w.view(np.int32).astype(np.int64))
        assert ulp.max(initial=0) <= 1 and (ulp != 0).mean() < 1e-3, (int(ulp.max()), float((ulp != 0).mean()))
    else:
        np.testing.assert_array_equal(w, r_w)
    if name == "dogleg":
        assert np.diff(ip).max() > 2000                     # the rows at the radar went through the ring

    radar = scene["vol"].as_radar()
    gf = rg.GateFilter(radar).exclude_below(*sc.QC)
    for f in sc.FIELDS:
        fdata = rg.get_field_data(radar, f)
        data, mask, _ = scene["host"][f]
        scale = float(np.nanmax(np.abs(data[~mask])))
        assert_same_to_rounding(rg.apply_geometry(geom, fdata), ref[f"{name}_grid_{f}"], scale)
        assert_same_to_rounding(rg.apply_geometry(geom, fdata, additional_filters=[gf]), ref[f"{name}_grid_{f}_qc"], scale)
        assert_same_to_rounding(rg.apply_geometry(geom, fdata, additional_filters=[gf], fill_value=sc.FILL),
                                ref[f"{name}_grid_{f}_qc_fill"], scale, fill=sc.FILL)


def test_section_geometry_is_an_ordinary_geometry(rg, scene, tmp_path):
    """apply_geometry_multi, grid_fields_device and save_geometry / load_geometry take it unchanged."""
    name, weighting = "dogleg", "barnes2"
    _, ref = sc.fixture(weighting)
    xs, ys, _ = sc.path_points(name)
    geom = rg.compute_section_geometry(scene["search"], xs, ys, weighting)
    radar = scene["vol"].as_radar()
    gf = rg.GateFilter(radar).exclude_below(*sc.QC)
    fields = {f: rg.get_field_data(radar, f) for f in sc.FIELDS}
    scale = {f: float(np.nanmax(np.abs(scene["host"][f][0][~scene["host"][f][1]]))) for f in sc.FIELDS}
    multi = rg.apply_geometry_multi(geom, fields, additional_filters={f: [gf] for f in sc.FIELDS})
    for f in sc.FIELDS:
        assert multi[f].shape == geom.grid_shape
        assert_same_to_rounding(multi[f], ref[f"{name}_grid_{f}_qc"], scale[f])
    dev_out = rg.grid_fields_device(geom, [scene["f"][f] for f in sc.FIELDS], [scene["m"][f] for f in sc.FIELDS])
    for k, f in enumerate(sc.FIELDS):
        assert_same_to_rounding(dev_out[k].reshape(geom.grid_shape), ref[f"{name}_grid_{f}"], scale[f])
    path = str(tmp_path / "section.npz")
    rg.save_geometry(geom, path)
    back = rg.load_geometry(path)
    assert tuple(back.grid_shape) == geom.grid_shape
    np.testing.assert_array_equal(back.indptr, geom.indptr)
    np.testing.assert_array_equal(back.gate_indices, geom.gate_indices)
    np.testing.assert_array_equal(back.weights, geom.weights)
    f = sc.FIELDS[0]
    np.testing.assert_array_equal(rg.apply_geometry(back, fields[f]), rg.apply_geometry(geom, fields[f]))


# ---- 2. the CSR-free route within the per-sample bound ---------------------------------------------------------------------
def path_window(xs, ys):
    """The smallest window of the scene's lattice whose coordinate range holds the points."""
    yc = oracle.axis_coords_f32(*sc.GRID_LIMITS[1], sc.GRID_SHAPE[1])
    xc = oracle.axis_coords_f32(*sc.GRID_LIMITS[2], sc.GRID_SHAPE[2])
    iy0 = int(np.searchsorted(yc, ys.min(), side="right")) - 1
    iy1 = int(np.searchsorted(yc, ys.max(), side="left")) + 1
    ix0 = int(np.searchsorted(xc, xs.min(), side="right")) - 1
    ix1 = int(np.searchsorted(xc, xs.max(), side="left")) + 1
    assert yc[iy0] <= ys.min() and ys.max() <= yc[iy1 - 1] and xc[ix0] <= xs.min() and xs.max() <= xc[ix1 - 1]
    return iy0, iy1, ix0, ix1


@pytest.mark.parametrize("weighting", sc.WEIGHTINGS)
@pytest.mark.parametrize("name", PATHS)
def test_section_fields_within_the_bound(rg, scene, name, weighting):
    import torch
    xs, ys, _ = sc.path_points(name)
    F = sc.FIELDS
    st = {(f, q): stats_of(scene, name, weighting, f, q) for f in F for q in (0, 1)}
    shape = (sc.NZ, len(xs))
    searches = [("default", scene["search"])] + [(str(kw), make_search(rg, scene, **kw)) for kw in SEARCHES[1:]]
    window = path_window(xs, ys)
    assert window != (0, sc.GRID_SHAPE[1], 0, sc.GRID_SHAPE[2])
    searches.append((f"window={window}", make_search(rg, scene, window=window)))
    for label, search in searches:
        got = rg.section_fields_device(search, xs, ys, [scene["f"][F[0]]], [scene["m"][F[0]]], weighting=weighting)
        assert tuple(got.shape) == (1,) + shape
        check_bound(name, weighting, got[0].cpu().numpy(), st[F[0], 0], f"{label} 1f")
        three = [F[k % len(F)] for k in range(3)]
        got = rg.section_fields_device(search, xs, ys, [scene["f"][f] for f in three], [scene["m"][f] for f in three],
                                       shared_mask=scene["qc_t"], weighting=weighting).cpu().numpy()
        for k, f in enumerate(three):
            check_bound(name, weighting, got[k], st[f, 1], f"{label} 3f_qc[{k}]")
        # 5 fields (stride 8): plain and QC-masked ones mixed through per-field masks
        five = [(F[k % len(F)], k % 2) for k in range(5)]
        qc_or = {f: torch.maximum(scene["m"][f], scene["qc_t"]) for f in F}
        got = rg.section_fields_device(search, xs, ys, [scene["f"][f] for f, _ in five],
                                       [qc_or[f] if q else scene["m"][f] for f, q in five], weighting=weighting,
                                       fill_value=sc.FILL).cpu().numpy()
        for k, (f, q) in enumerate(five):
            g = got[k].copy()
            np.testing.assert_array_equal(g == np.float32(sc.FILL), np.isnan(st[f, q]["m"]).reshape(shape))
            g[g == np.float32(sc.FILL)] = np.nan
            check_bound(name, weighting, g, st[f, q], f"{label} 5f[{k}]")


def test_more_than_eight_fields_go_in_groups(rg, scene):
    name, weighting = "diag", "cressman"
    xs, ys, _ = sc.path_points(name)
    F = sc.FIELDS
    ten = [F[k % len(F)] for k in range(10)]
    got = rg.section_fields_device(scene["search"], xs, ys, [scene["f"][f] for f in ten], [scene["m"][f] for f in ten],
                                   weighting=weighting).cpu().numpy()
    assert got.shape == (10, sc.NZ, len(xs))
    for k, f in enumerate(ten):
        check_bound(name, weighting, got[k], stats_of(scene, name, weighting, f, 0), f"10f[{k}]")


# ---- 3. lattice consistency, order independence, the host convenience -----------------------------------------------------
@pytest.mark.parametrize("weighting", sc.WEIGHTINGS)
def test_a_grid_row_as_a_section(rg, scene, weighting):
    search = scene["search"]
    nz, ny, nx = sc.GRID_SHAPE
    yc = oracle.axis_coords_f32(*sc.GRID_LIMITS[1], ny)
    xs = oracle.axis_coords_f32(*sc.GRID_LIMITS[2], nx)
    F = sc.FIELDS
    lattice = rg.roi_grid_fields_device(search, [scene["f"][f] for f in F], [scene["m"][f] for f in F], weighting=weighting)
    csr = search.build_csr(weighting)
    l_ip = csr.indptr.cpu().numpy().astype(np.int64)
    l_idx, l_w = csr.gate_indices.cpu().numpy(), csr.weights.cpu().numpy()
    for j in (3, 17, ny - 1):                               # row 17 passes 2 km from the radar
        ys = np.full(nx, yc[j], dtype=np.float32)
        got = rg.section_fields_device(search, xs, ys, [scene["f"][f] for f in F], [scene["m"][f] for f in F],
                                       weighting=weighting)
        for k, f in enumerate(F):
            data, mask, _ = scene["host"][f]
            assert_same_to_rounding(got[k], lattice[k, :, j, :], float(np.nanmax(np.abs(data[~mask]))))
        geom = rg.compute_section_geometry(search, xs, ys, weighting)
        rows = (np.arange(nz)[:, None] * ny + j) * nx + np.arange(nx)[None, :]
        lengths = (l_ip[rows + 1] - l_ip[rows]).ravel()
        pick = np.concatenate([np.arange(l_ip[r], l_ip[r + 1]) for r in rows.ravel()]) if lengths.sum() else np.zeros(0, np.int64)
        want = oracle.canonical_rows(np.concatenate([[0], np.cumsum(lengths)]), l_idx[pick], l_w[pick])
        have = oracle.canonical_rows(geom.indptr, geom.gate_indices, geom.weights)
        assert want[0][-1] > 0
        for a, b in zip(have, want):
            np.testing.assert_array_equal(a, b)             # the same code weighs both: the weights are equal too


@pytest.mark.parametrize("weighting", sc.WEIGHTINGS)
def test_the_order_of_the_points_does_not_matter(rg, scene, weighting):
    name = "dogleg"
    xs, ys, _ = sc.path_points(name)
    perm = np.random.default_rng(1234).permutation(len(xs))
    f = sc.FIELDS[0]
    args = ([scene["f"][f]], [scene["m"][f]])
    straight = rg.section_fields_device(scene["search"], xs, ys, *args, weighting=weighting)[0].cpu().numpy()
    shuffled = rg.section_fields_device(scene["search"], xs[perm], ys[perm], *args, weighting=weighting)[0].cpu().numpy()
    np.testing.assert_array_equal(np.isnan(shuffled), np.isnan(straight[:, perm]))
    st = stats_of(scene, name, weighting, f, 0)
    st_perm = {k: np.asarray(v).reshape(sc.NZ, len(xs))[:, perm].ravel() for k, v in st.items()}
    check_bound(name, weighting, shuffled, st_perm, "shuffled")
    geom = rg.compute_section_geometry(scene["search"], xs[perm], ys[perm], weighting)
    lengths = np.diff(sc.scene_pairs(name)[0]).reshape(sc.NZ, len(xs))
    np.testing.assert_array_equal(np.diff(geom.indptr.astype(np.int64)).reshape(sc.NZ, len(xs)), lengths[:, perm])


@pytest.mark.parametrize("weighting", sc.WEIGHTINGS)
@pytest.mark.parametrize("name", PATHS)
def test_vertical_section_end_to_end(rg, scene, name, weighting):
    """NumPy in, NumPy out: a search structure of its own, built for the path's bounding box.  Against the fixture: the
    reference's fill pattern, and every sample within the bound around the float64 mean of the reference's neighbours."""
    _, ref = sc.fixture(weighting)
    vol = scene["vol"]
    radar = vol.as_radar()
    gf = rg.GateFilter(radar).exclude_below(*sc.QC)
    vertices, spacing = sc.PATHS[name]
    f = sc.FIELDS[0]
    got, s = rg.vertical_section(vol.gate_x, vol.gate_y, vol.gate_z, rg.get_field_data(radar, f), vertices, spacing,
                                 sc.Z_LIMITS, sc.NZ, additional_filters=[gf], weighting=weighting, toa=sc.TOA)
    want = ref[f"{name}_grid_{f}_qc"]
    assert got.dtype == np.float32 and got.shape == (sc.NZ, len(s)) == want.reshape(sc.NZ, -1).shape
    np.testing.assert_array_equal(s, ref[f"{name}_s"])
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want.reshape(got.shape)))
    check_bound(name, weighting, got, stats_of(scene, name, weighting, f, 1), "vertical_section")
    got_fill, _ = rg.vertical_section(vol.gate_x, vol.gate_y, vol.gate_z, rg.get_field_data(radar, f), vertices, spacing,
                                      sc.Z_LIMITS, sc.NZ, additional_filters=[gf], weighting=weighting, toa=sc.TOA,
                                      fill_value=sc.FILL)
    np.testing.assert_array_equal(got_fill == np.float32(sc.FILL), np.isnan(got))


def test_a_path_along_an_axis(rg, scene):
    """A rectangle of zero width is legal: a north-south line through the radar."""
    vol = scene["vol"]
    f = sc.FIELDS[0]
    vertices, spacing = [(0.0, -30e3), (0.0, 30e3)], 750.0
    got, s = rg.vertical_section(vol.gate_x, vol.gate_y, vol.gate_z, vol.fields[f], vertices, spacing, sc.Z_LIMITS, 6,
                                 weighting="nearest", toa=sc.TOA)
    xs, ys, _ = rg.section_path(vertices, spacing)
    assert np.all(xs == 0.0) and got.shape == (6, len(s)) == (6, 81)
    ip, idx, w64 = sc.brute_section(vol.gate_x, vol.gate_y, vol.gate_z, xs, ys, sc.levels(nz=6), "nearest", exact_weights=True)
    data, mask, _ = scene["host"][f]
    r = oracle.bound_ratio(got, oracle.voxel_stats(ip, idx, w64, data, mask), oracle.DELTA_K2["nearest"])
    assert r.max(initial=0.0) <= 1.0 and np.diff(ip).max() > 1000
