"""A vertical section through a mosaic on the MI355X (rg_roi_section_mosaic_f32 and the Python surface over it), on the
scenes of tests/mosaic_section_scenes.py: 16 radars (12 live, 4 inert), a dog-leg of 193 points x 5 levels.

 1. ``mosaic_section_fields_device`` on a lattice ``MosaicSearch`` and on a ``for_path`` one: the oracle's fill pattern and
    ``bound_ratio <= 1`` (oracle.DELTA_K2) around the float64 mean of the union of every radar's brute-force neighbours.
 2. Bit identities: one radar alone is ``section_fields_device`` on that radar's search; a one-entry table is
    ``rg_roi_section_f32``; inert radars change no bit.
 3. Subsets of the radars.  4. A row of the lattice mosaic as a section.  5. The geometry route against the reference's
    fixtures (g12_mosaic_section_*) and, with 20 radars, the float64 mean.  6. The NumPy convenience.

One radar alone against the single-radar section, bit for bit: a block of the section kernel is 4 consecutive points, and
which queue slot adds a hit to a point's sums depends on the survivors of the block's other points (that is why
test_gpu_section.py compares shuffled points within the bound, not bit for bit).  The NaN points are therefore removed
block-wise: a block without a live point is dropped whole, and a dead point of a mixed block is replaced by a copy of a
live point of the same block -- a duplicate adds no candidate (its sub-box is the other's), so every live point keeps its
block, its queue and its bits; the copies' samples are discarded.  (Measured on this scene with the dead points removed one by
one instead: 890 / 878 / 523 of 3017 filled samples differ in bits for barnes2 / cressman / nearest, by at most 3.4e-7
relative -- the regrouped blocks, not the radar-visit loop.)"""
import json
import os

import numpy as np
import pytest

import mosaic_scenes as ms
import mosaic_section_scenes as mss
from conftest import assert_same_to_rounding
from oracle import radar_grid_oracle as oracle

pytestmark = pytest.mark.gpu

WEIGHTINGS = mss.WEIGHTINGS
REPORT = {}
FILL = mss.FILL


@pytest.fixture(scope="module")
def env():
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native
    rg.load_library()
    return dict(torch=torch, rg=rg, native=_native, dev=torch.device("cuda", 0), cache={})


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    print("mosaic_section_bounds", json.dumps(REPORT, sort_keys=True))
    out_dir = os.environ.get("RG_REPORT_DIR")
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "mosaic_section_bounds.json"), "w") as fh:
            json.dump(REPORT, fh, indent=1, sort_keys=True)


def _dev(env, a, dtype=None):
    torch = env["torch"]
    return torch.from_numpy(np.ascontiguousarray(a)).to(env["dev"], dtype=dtype or torch.float32)


def _search(env, scene, kind):
    """The scene's MosaicSearch, built once: ``lattice`` (reach windows on the scene's grid) or ``path`` (for_path)."""
    key = (scene.name, kind)
    if key not in env["cache"]:
        rg = env["rg"]
        xs, ys, _ = mss.path()
        kw = dict(min_radius=scene.min_radius, beam_factor=scene.beam_factor, toa=scene.toa)
        if kind == "lattice":
            env["cache"][key] = rg.MosaicSearch(scene.radars(), scene.shape, scene.limits, **kw)
        else:
            env["cache"][key] = rg.MosaicSearch.for_path(scene.radars(), xs, ys, scene.limits[0], scene.shape[0], **kw)
    return env["cache"][key]


def _field_set(scene, nf):
    """Per radar ``nf`` (values, mask) pairs -- field k is FIELDS[k % 3] of the radar plus k with the field's own mask (all
    gates for the 'masked' radar) -- and the radar's QC mask (RHOHV below 0.8)."""
    out, shared = [], []
    for v in scene.vols:
        n = len(v.gate_x)
        shared.append(oracle.gate_mask("below", np.ma.getdata(v.fields["RHOHV"]), 0.8) if n else np.zeros(0, dtype=bool))
        out.append([((np.ma.getdata(v.fields[ms.FIELDS[k % 3]]) + np.float32(k)).astype(np.float32),
                     np.ma.getmaskarray(v.fields[ms.FIELDS[k % 3]]).copy()) for k in range(nf)])
    return out, shared


def _device_call(env, fs, shared, sel, with_shared=True):
    torch = env["torch"]
    fields = [[_dev(env, d) for d, _ in fs[r]] for r in sel]
    masks = [[_dev(env, m.astype(np.uint8), torch.uint8) for _, m in fs[r]] for r in sel]
    shared_t = [_dev(env, shared[r].astype(np.uint8), torch.uint8) for r in sel] if with_shared else None
    return fields, masks, shared_t


def _stats(scene, weighting, fs, shared, k, sel=None, with_shared=True, **points):
    sel = list(range(scene.n_radars)) if sel is None else list(sel)
    ip, idx, w64 = mss.mosaic_csr(scene, weighting, sel, **points)
    data = np.concatenate([fs[r][k][0] for r in sel])
    mask = np.concatenate([fs[r][k][1] | shared[r] if with_shared else fs[r][k][1] for r in sel])
    return oracle.voxel_stats(ip, idx, w64, data, mask)


def _check(got, stats, weighting, label, shape, delta=None, min_filled=150):
    """``got`` was gridded with fill -9999: the fill pattern is the oracle's, every sample lies within the bound."""
    got = (got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)).reshape(shape).copy()
    empty = np.isnan(stats["m"]).reshape(shape)
    assert (~empty).sum() >= min_filled, (label, int((~empty).sum()))          # the comparison is not vacuous
    np.testing.assert_array_equal(got == np.float32(FILL), empty, err_msg=label)
    got[empty] = np.nan
    ratio = oracle.bound_ratio(got, stats, oracle.DELTA_K2[weighting] if delta is None else delta)
    worst = float(ratio.max(initial=0.0))
    print(f"{label}: worst bound ratio {worst:.4f} over {int((~empty).sum())} filled samples")
    REPORT[weighting] = max(REPORT.get(weighting, 0.0), worst)
    assert worst <= 1.0, (label, worst, int((ratio > 1).sum()))


# ---- 1. the bound -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lattice", "path"])
@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_mosaic_section_within_the_bound(env, weighting, kind):
    rg = env["rg"]
    scene = ms.scene16()
    xs, ys, _ = mss.path()
    search = _search(env, scene, kind)
    shape = (scene.shape[0], len(xs))
    sel = list(range(scene.n_radars))
    if kind == "path":      # a search exactly where path_reach says so; the three inert radars without valid gates have none
        box = (float(xs.min()), float(xs.max()), float(ys.min()), float(ys.max()))
        reach = [rg.path_reach(v.gate_x, v.gate_y, v.gate_z, o, box, scene.min_radius, scene.beam_factor, scene.toa)
                 for v, o in zip(scene.vols, scene.origins)]
        assert [s is not None for s in search.searches] == reach
        assert all(search.searches[r] is None for r, k in enumerate(scene.kinds) if k in ("far", "no_gates", "above_toa"))
        assert sum(reach) == 13 and search.grid_shape == (scene.shape[0], 2, 2)
        assert all(s.window == (0, 2, 0, 2) and s.grid_shape == search.grid_shape for s in search.searches if s is not None)
    for nf, with_shared in ((1, False), (3, True), (5, False)):
        fs, shared = _field_set(scene, nf)
        fields, masks, shared_t = _device_call(env, fs, shared, sel, with_shared)
        got = rg.mosaic_section_fields_device(search, xs, ys, fields, masks, shared_t, weighting=weighting, fill_value=FILL)
        assert tuple(got.shape) == (nf,) + shape and got.dtype == env["torch"].float32
        for k in range(nf):
            _check(got[k], _stats(scene, weighting, fs, shared, k, with_shared=with_shared), weighting,
                   f"{kind} {weighting} {nf} field(s), field {k}", shape)


def test_more_than_eight_fields_go_in_groups(env):
    rg = env["rg"]
    scene = ms.scene16()
    xs, ys, _ = mss.path()
    fs, shared = _field_set(scene, 10)
    sel = list(range(scene.n_radars))
    got = rg.mosaic_section_fields_device(_search(env, scene, "path"), xs, ys, *_device_call(env, fs, shared, sel),
                                          weighting="cressman", fill_value=FILL)
    assert tuple(got.shape) == (10, scene.shape[0], len(xs))
    for k in (0, 7, 8, 9):
        _check(got[k], _stats(scene, "cressman", fs, shared, k), "cressman", f"10 fields, field {k}", got.shape[1:])


# ---- 2. bit identities -------------------------------------------------------------------------------------------------------
def _without_dead_points(x_r, y_r):
    """The points with the NaN ones removed block-wise (module docstring): ``(xs, ys, keep)`` -- ``keep[j]`` the original
    point whose sample column j of the result is, or -1 for the copy of a live point that stands in for a dead one."""
    xs, ys, keep = [], [], []
    for b0 in range(0, len(x_r), 4):
        idx = np.arange(b0, min(b0 + 4, len(x_r)))
        live = idx[~np.isnan(x_r[idx])]
        if live.size == 0:
            continue
        for i in idx:
            j = i if not np.isnan(x_r[i]) else live[0]
            xs.append(x_r[j]); ys.append(y_r[j]); keep.append(i if j == i else -1)
    return np.float32(xs), np.float32(ys), np.asarray(keep)


@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_one_radar_alone_is_the_single_radar_section(env, weighting):
    rg, torch = env["rg"], env["torch"]
    scene = ms.scene16()
    xs, ys, _ = mss.path()
    search = _search(env, scene, "lattice")
    points = rg.mosaic_section_points(search, xs, ys)
    fs, shared = _field_set(scene, 3)
    live = [r for r, k in enumerate(scene.kinds) if k == "live"]
    mixed_blocks = finite = 0
    for r in live:
        fields, masks, shared_t = _device_call(env, fs, shared, [r])
        got = rg.mosaic_section_fields_device(search, xs, ys, fields, masks, shared_t, weighting=weighting, radars=[r])
        got = got.cpu().numpy()
        x_r, y_r = points[r]
        dead = np.isnan(x_r)
        assert np.isnan(got[:, :, dead]).all()
        if dead.all():
            continue
        cx, cy, keep = _without_dead_points(x_r, y_r)
        mixed_blocks += int((keep == -1).sum() > 0)
        want = rg.section_fields_device(search.searches[r], cx, cy, fields[0], masks[0], shared_mask=shared_t[0],
                                        weighting=weighting).cpu().numpy()
        np.testing.assert_array_equal(got[:, :, keep[keep >= 0]].view(np.int32), want[:, :, keep >= 0].view(np.int32),
                                      err_msg=f"radar {r}")
        finite += int(np.isfinite(want).sum())
    assert finite > 3 * 300 and mixed_blocks >= 4                        # windows' edges fall inside blocks, not only between them


@pytest.mark.parametrize("kind", ["lattice", "path"])
@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_one_entry_returns_the_bits_of_rg_roi_section(env, weighting, kind):
    """The C entry points side by side: a one-entry table with gate_offset 0 against rg_roi_section_f32 on the same search
    structure and the same (NaN-marked) points, for 1, 3 and 8 fields; through the ring (rows of hundreds of gates)."""
    rg, torch, native = env["rg"], env["torch"], env["native"]
    from radar_processor_amd.roi_grid import pack_and_grid
    scene = ms.scene16()
    xs, ys, _ = mss.path()
    search = _search(env, scene, kind)
    lib = native.load_library()
    r = max((r for r, k in enumerate(scene.kinds) if k == "live"), key=lambda r: int(np.diff(mss.radar_pairs(scene, r)[0]).max()))
    assert np.diff(mss.radar_pairs(scene, r)[0]).max() > 256
    s = search.searches[r]
    x_r, y_r = rg.mosaic_section_points(search, xs, ys)[r]
    assert np.isnan(x_r).any() == (kind == "lattice")
    pts = (_dev(env, x_r), _dev(env, y_r))
    nz, n = s.grid_shape[0], len(xs)
    for nf in (1, 3, 8):
        fs, shared = _field_set(scene, nf)
        fields, masks, shared_t = _device_call(env, fs, shared, [r])
        table = search.section_table([r], [0], [pts])
        outs = []
        for which in ("mosaic", "single"):
            def launch(packed, nf_, stride, out_view, stream):
                if which == "mosaic":
                    rc = lib.rg_roi_section_mosaic_f32(table, 1, nz, n, s.min_radius, s.beam_factor,
                                                       native.WEIGHTINGS[weighting], native.ptr(packed), nf_, stride,
                                                       s.n_gates, float("nan"), native.ptr(out_view), stream)
                else:
                    rc = lib.rg_roi_section_f32(native.ptr(s.sorted_gates), native.ptr(s.cell_start), s.cells,
                                                native.ptr(pts[0]), native.ptr(pts[1]), native.ptr(s.zc), nz, n, s.min_radius,
                                                s.beam_factor, native.WEIGHTINGS[weighting], native.ptr(packed), nf_, stride,
                                                float("nan"), native.ptr(out_view), stream)
                native.check(rc, which)
            outs.append(pack_and_grid(env["dev"], s.n_gates, fields[0], masks[0], shared_t[0], None, (nz, n), launch)
                        .cpu().numpy())
        assert np.isfinite(outs[1]).sum() > 50 * nf
        np.testing.assert_array_equal(outs[0].view(np.int32), outs[1].view(np.int32))
    # origin (0, 0, 0): the Python surfaces side by side
    v = scene.vols[r]
    one = rg.MosaicSearch.for_path([(v.gate_x, v.gate_y, v.gate_z, (0.0, 0.0, 0.0))], x_r[~np.isnan(x_r)], y_r[~np.isnan(x_r)],
                                   rg.mosaic_limits(scene.limits, scene.origins[r])[0], nz, min_radius=scene.min_radius,
                                   beam_factor=scene.beam_factor, toa=scene.toa - scene.origins[r][0])
    fs, shared = _field_set(scene, 2)
    fields, masks, shared_t = _device_call(env, fs, shared, [r])
    cx, cy = x_r[~np.isnan(x_r)], y_r[~np.isnan(x_r)]
    a = rg.mosaic_section_fields_device(one, cx, cy, fields, masks, shared_t, weighting=weighting).cpu().numpy()
    b = rg.section_fields_device(one.searches[0], cx, cy, fields[0], masks[0], shared_mask=shared_t[0],
                                 weighting=weighting).cpu().numpy()
    np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("kind", ["lattice", "path"])
@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_inert_radars_change_no_bit(env, weighting, kind):
    rg = env["rg"]
    scene = ms.scene16()
    xs, ys, _ = mss.path()
    search = _search(env, scene, kind)
    fs, shared = _field_set(scene, 3)
    live = [r for r, k in enumerate(scene.kinds) if k == "live"]
    assert len(live) == scene.n_radars - 4
    every = rg.mosaic_section_fields_device(search, xs, ys, *_device_call(env, fs, shared, range(scene.n_radars)),
                                            weighting=weighting).cpu().numpy()
    only_live = rg.mosaic_section_fields_device(search, xs, ys, *_device_call(env, fs, shared, live), weighting=weighting,
                                                radars=live).cpu().numpy()
    assert np.isfinite(every).sum() > 3 * 150
    np.testing.assert_array_equal(every.view(np.int32), only_live.view(np.int32))


# ---- 3. subsets ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_subsets_of_the_radars(env, weighting):
    rg = env["rg"]
    scene = ms.scene16()
    xs, ys, _ = mss.path()
    shape = (scene.shape[0], len(xs))
    cluster = [1, 4, 5, 8, 9, 12, 13, 15]                  # mosaic_scenes._specs16: the eight radars around one point
    rim = [2, 6, 10, 14]
    assert sorted(cluster + rim) == [r for r, k in enumerate(scene.kinds) if k == "live"]
    fs, shared = _field_set(scene, 2)
    for kind in ("lattice", "path"):
        search = _search(env, scene, kind)
        for name, sel, floor in (("cluster", cluster, 100), ("rim", rim, 50), ("rim then cluster, reversed", (rim + cluster)[::-1], 150)):
            got = rg.mosaic_section_fields_device(search, xs, ys, *_device_call(env, fs, shared, sel), weighting=weighting,
                                                  fill_value=FILL, radars=sel)
            for k in range(2):
                _check(got[k], _stats(scene, weighting, fs, shared, k, sel), weighting, f"{kind} {name} field {k}", shape,
                       min_filled=floor)


# ---- 4. a row of the lattice mosaic as a section -----------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_a_lattice_row_as_a_mosaic_section(env, weighting):
    """scene3's origins are whole metres on the 3 km lattice: the section's points in a radar's frame ARE that radar's voxel
    coordinates, so a row of mosaic_fields_device and the section along it see the same neighbours -- the same fill pattern,
    each within its own bound of the same float64 mean."""
    rg = env["rg"]
    scene = mss.scene3()
    nz, ny, nx = scene.shape
    search = rg.MosaicSearch(scene.radars(), scene.shape, scene.limits, min_radius=scene.min_radius,
                             beam_factor=scene.beam_factor, toa=scene.toa)
    yc = oracle.axis_coords_f32(*scene.limits[1], ny)
    xs = oracle.axis_coords_f32(*scene.limits[2], nx)
    fs, shared = _field_set(scene, 2)
    sel = list(range(scene.n_radars))
    call = _device_call(env, fs, shared, sel)
    lattice = rg.mosaic_fields_device(search, *call, weighting=weighting, fill_value=FILL).cpu().numpy()
    filled = 0
    for j in (7, 11, 15):                                  # the rows nearest radar 2, radar 0 and radar 1
        ys = np.full(nx, yc[j], dtype=np.float32)
        got = rg.mosaic_section_fields_device(search, xs, ys, *call, weighting=weighting, fill_value=FILL).cpu().numpy()
        np.testing.assert_array_equal(got == np.float32(FILL), lattice[:, :, j, :] == np.float32(FILL))
        for k in range(2):
            stats = _stats(scene, weighting, fs, shared, k, sel, xs=xs, ys=ys, key=f"row{j}")
            filled += int((~np.isnan(stats["m"])).sum())
            _check(got[k], stats, weighting, f"section along row {j}, field {k}", (nz, nx), min_filled=0)
            _check(lattice[k, :, j, :], stats, weighting, f"lattice row {j}, field {k}", (nz, nx), min_filled=0)
    assert filled >= 100


# ---- 5. the geometry route -----------------------------------------------------------------------------------------------------
def _section_geometry(env, scene, weighting):
    key = ("geometry", scene.name, weighting)
    if key not in env["cache"]:
        xs, ys, _ = mss.path()
        env["cache"][key] = env["rg"].compute_mosaic_section_geometry(
            scene.radars(), xs, ys, scene.limits[0], scene.shape[0], min_radius=scene.min_radius,
            beam_factor=scene.beam_factor, weighting=weighting, toa=scene.toa)
    return env["cache"][key]


def _masked_fields(rg, scene, name):
    """Per radar the masked field and a GateFilter list with the fixtures' QC filter (none for the radar without gates)."""
    fields = [np.ma.array(np.ma.getdata(v.fields[name]), mask=np.ma.getmaskarray(v.fields[name])) for v in scene.vols]
    filters = [[rg.GateFilter(v.as_radar()).exclude_below(*mss.QC)] if len(v.gate_x) else [] for v in scene.vols]
    return fields, filters


@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_section_geometry_matches_the_reference(env, weighting, tmp_path):
    rg = env["rg"]
    scene = ms.scene16()
    xs, ys, s = mss.path()
    _, ref = mss.fixture(weighting)
    geom = _section_geometry(env, scene, weighting)
    nz, n = scene.shape[0], len(xs)
    assert geom.grid_shape == (nz, 1, n) and geom.toa == scene.toa
    s_last = float(np.hypot(np.diff(xs.astype(np.float64)), np.diff(ys.astype(np.float64))).sum())
    assert geom.grid_limits == (tuple(float(v) for v in scene.limits[0]), (0.0, 0.0), (0.0, s_last))
    np.testing.assert_array_equal(geom.section_x, xs)
    np.testing.assert_array_equal(geom.section_y, ys)
    np.testing.assert_array_equal(geom.gate_offsets, scene.offsets())
    np.testing.assert_array_equal(geom.origins, np.asarray(scene.origins, dtype=np.float64))
    # row = radar 0's row, then radar 1's, ...: the fixture's row layout, pair by pair
    np.testing.assert_array_equal(np.asarray(geom.indptr, dtype=np.int64), ref["indptr"].astype(np.int64))
    radar_of = np.searchsorted(scene.offsets(), np.asarray(geom.gate_indices, dtype=np.int64), side="right") - 1
    row_of = np.repeat(np.arange(nz * n), np.diff(np.asarray(geom.indptr, dtype=np.int64)))
    assert np.all((np.diff(radar_of) >= 0) | (np.diff(row_of) > 0))
    ip, idx, w = oracle.canonical_rows(geom.indptr, geom.gate_indices, geom.weights)
    r_ip, r_idx, r_w = oracle.canonical_rows(ref["indptr"], ref["gate_indices"], ref["weights"])
    np.testing.assert_array_equal(ip, r_ip)
    np.testing.assert_array_equal(idx, r_idx)
    if weighting == "barnes2":
        ulp = np.abs(w.view(np.int32).astype(np.int64) - r_w.view(np.int32).astype(np.int64))
        assert ulp.max(initial=0) <= 1 and (ulp != 0).mean() < 1e-3, (int(ulp.max()), float((ulp != 0).mean()))
    else:
        np.testing.assert_array_equal(w, r_w)
    assert np.diff(ip).max() > 1000                          # eight radars' rows, one after the other
    # apply_mosaic / apply_mosaic_multi / mosaic_fields_device / save_geometry take it unchanged
    for f in mss.FIELDS:
        fields, filters = _masked_fields(rg, scene, f)
        data, mask = mss.concat_field(scene, f)
        scale = float(np.nanmax(np.abs(data[~mask])))
        got = rg.apply_mosaic(geom, fields)
        assert got.shape == geom.grid_shape and got.dtype == np.float32
        assert_same_to_rounding(got, ref[f"grid_{f}"], scale)
        assert_same_to_rounding(rg.apply_mosaic(geom, fields, filters), ref[f"grid_{f}_qc"], scale)
        assert_same_to_rounding(rg.apply_mosaic(geom, fields, filters, fill_value=FILL), ref[f"grid_{f}_qc_fill"], scale,
                                fill=FILL)
    if weighting == "barnes2":
        multi = rg.apply_mosaic_multi(geom, {f: _masked_fields(rg, scene, f)[0] for f in mss.FIELDS},
                                      {f: _masked_fields(rg, scene, f)[1] for f in mss.FIELDS})
        fs, shared = _field_set(scene, 1)
        dev_out = rg.mosaic_fields_device(geom, *_device_call(env, fs, shared, range(scene.n_radars), with_shared=False))
        for f in mss.FIELDS:
            data, mask = mss.concat_field(scene, f)
            assert_same_to_rounding(multi[f], ref[f"grid_{f}_qc"], float(np.nanmax(np.abs(data[~mask]))))
        data, mask = mss.concat_field(scene, ms.FIELDS[0])
        assert ms.FIELDS[0] == mss.FIELDS[0]
        assert_same_to_rounding(dev_out[0].cpu().numpy().reshape(geom.grid_shape), ref[f"grid_{ms.FIELDS[0]}"],
                                float(np.nanmax(np.abs(data[~mask]))))
        path = str(tmp_path / "mosaic_section.npz")
        rg.save_geometry(geom, path)
        back = rg.load_geometry(path)
        assert tuple(back.grid_shape) == geom.grid_shape
        np.testing.assert_array_equal(back.indptr, geom.indptr)
        np.testing.assert_array_equal(back.gate_indices, geom.gate_indices)
        np.testing.assert_array_equal(back.weights, geom.weights)


@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_twenty_radars_through_the_geometry_route(env, weighting):
    """More radars than one CSR-free launch takes: rows against the oracle's, grids against the float64 mean."""
    rg = env["rg"]
    scene = ms.scene20()
    xs, ys, _ = mss.path()
    geom = _section_geometry(env, scene, weighting)
    ip, idx, w = mss.mosaic_csr(scene, weighting, exact=False)
    np.testing.assert_array_equal(np.asarray(geom.indptr, dtype=np.int64), ip)
    have = oracle.canonical_rows(geom.indptr, geom.gate_indices, geom.weights)
    want = oracle.canonical_rows(ip, idx, w)
    np.testing.assert_array_equal(have[1], want[1])
    assert int(ip[-1]) > int(mss.mosaic_csr(ms.scene16(), weighting, exact=False)[0][-1])      # the four extra radars add pairs
    with pytest.raises(ValueError, match="at most 16"):
        rg.MosaicSearch.for_path(scene.radars(), xs, ys, scene.limits[0], scene.shape[0])
    shape = (scene.shape[0], len(xs))
    fs, shared = _field_set(scene, 3)
    sel = list(range(scene.n_radars))
    got = rg.mosaic_fields_device(geom, *_device_call(env, fs, shared, sel), fill_value=FILL)
    for k in range(3):
        _check(got[k], _stats(scene, weighting, fs, shared, k), weighting, f"scene20 geometry route, field {k}", shape,
               delta=oracle.DELTA_CSR[weighting])


# ---- 6. NumPy in, NumPy out ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_mosaic_vertical_section_is_the_device_call_on_a_path_search(env, weighting):
    rg, torch = env["rg"], env["torch"]
    from radar_processor_amd.gridding import _coerce_filters, _host_field
    scene = ms.scene16()
    xs, ys, s = mss.path()
    f = mss.FIELDS[0]
    fields, filters = _masked_fields(rg, scene, f)
    got, dist = rg.mosaic_vertical_section(scene.radars(), fields, mss.VERTICES, mss.SPACING, scene.limits[0], scene.shape[0],
                                           additional_filters=filters, min_radius=scene.min_radius,
                                           beam_factor=scene.beam_factor, weighting=weighting, toa=scene.toa)
    assert got.dtype == np.float32 and got.shape == (scene.shape[0], len(xs))
    np.testing.assert_array_equal(dist, s)
    host = [_host_field(fields[r], _coerce_filters(filters[r])) for r in range(scene.n_radars)]
    f_t = [[_dev(env, v)] for v, _ in host]
    m_t = [[_dev(env, m.astype(np.uint8), torch.uint8)] for _, m in host]
    want = rg.mosaic_section_fields_device(_search(env, scene, "path"), xs, ys, f_t, m_t, weighting=weighting)[0].cpu().numpy()
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))
    # ... with the reference's fill pattern, every sample within the bound around the float64 mean
    _, ref = mss.fixture(weighting)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref[f"grid_{f}_qc"].reshape(got.shape)))
    ip, idx, w64 = mss.mosaic_csr(scene, weighting)
    data, mask_qc = mss.concat_field(scene, f, qc=True)
    ratio = oracle.bound_ratio(got, oracle.voxel_stats(ip, idx, w64, data, mask_qc), oracle.DELTA_K2[weighting])
    assert np.isfinite(got).sum() > 150 and ratio.max(initial=0.0) <= 1.0, float(ratio.max())
    got_fill, _ = rg.mosaic_vertical_section(scene.radars(), fields, mss.VERTICES, mss.SPACING, scene.limits[0],
                                             scene.shape[0], additional_filters=filters, min_radius=scene.min_radius,
                                             beam_factor=scene.beam_factor, weighting=weighting, toa=scene.toa, fill_value=FILL)
    np.testing.assert_array_equal(got_fill == np.float32(FILL), np.isnan(got))
