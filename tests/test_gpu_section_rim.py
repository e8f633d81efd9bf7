"""The section kernel (csrc/rg_roi_section.hip) at the ROI rim and on adversarial point sets: the scenes of
tests/section_rim_scenes.py against ``section_scenes.brute_pairs`` -- a float64 loop over all gates, no search structure.

What only the section kernel has, and what here would notice it being subtly wrong: the pre-filter (distance to the nearest
of four sub-boxes against the block's largest radius inflated by the rim band: gates in the outermost 2e-6 of a rim, points
of one block far apart, four radii in one block), the block's cell box (wave reductions, dead lanes, more than 64 cell rows),
the 4 x 16 lane layout (per-point decisions inside one block, duplicates, ragged tails), dead lanes (non-finite points
through the C ABI), the ring (rows of 600 neighbours) and the mosaic's visit loop (a rim cloud in a shifted frame).

 1. Builder: ``compute_section_geometry`` after oracle.canonical_rows equals ``brute_section``: row pointers and index sets
    exactly, Cressman and uniform weights bit for bit, Barnes within one ulp (the rule of test_gpu_roi_rim._check_csr).
 2. Gridder: ``section_fields_device``: the oracle's NaN pattern, every value inside the range of its sample's unmasked
    neighbours (test_gpu_roi_rim._check_grid) and within oracle.mean_error_bound (DELTA_K2) of the float64 mean.
Both for every RoiSearch variant of test_gpu_roi_rim.SEARCHES.  The worst err / bound per scene and weighting is printed
as one JSON line and written to section_rim_bounds.json where RG_REPORT_DIR names a directory."""
import functools
import json
import os

import numpy as np
import pytest

import mosaic_scenes as ms
import mosaic_section_scenes as mss
import section_rim_scenes as srs
import section_scenes as sc
from oracle import radar_grid_oracle as oracle
from oracle import roi_rim
from test_gpu_mosaic import _segments
from test_gpu_roi_rim import SEARCHES, _check_grid, _values_and_mask

pytestmark = pytest.mark.gpu

WEIGHTINGS = srs.WEIGHTINGS
REPORT = {}
FILL = -9999.0
_SEARCH_CACHE = {}              # (scene key, variant) -> RoiSearch, shared by the weightings


@pytest.fixture(scope="module")
def env():
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native
    rg.load_library()
    return dict(torch=torch, rg=rg, native=_native, dev=torch.device("cuda", 0))


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    _SEARCH_CACHE.clear()
    print("section_rim_bounds", json.dumps(REPORT, sort_keys=True))
    out_dir = os.environ.get("RG_REPORT_DIR")
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "section_rim_bounds.json"), "w") as fh:
            json.dump(REPORT, fh, indent=1, sort_keys=True)


def _dev(env, a, dtype=None):
    torch = env["torch"]
    return torch.from_numpy(np.ascontiguousarray(a)).to(env["dev"], dtype=dtype or torch.float32)


def _search(env, key, s, gates, variant):
    """The scene's RoiSearch over ``gates`` for SEARCHES[variant], built once per (key, variant)"""
    if (key, variant) not in _SEARCH_CACHE:
        kw = SEARCHES[variant]
        search = env["rg"].RoiSearch(*gates, s.grid_shape, s.grid_limits, radar_altitude=0.0, device=env["dev"],
                                     window=s.window, **s.roi, **kw)
        if "per_level" in kw:
            assert search.per_level == kw["per_level"]
        _SEARCH_CACHE[key, variant] = search
    return _SEARCH_CACHE[key, variant]


def _assert_coverage(name):
    cloud, need = srs.cloud(name), srs.scene(name).need
    counts = cloud.counts()
    print(f"{name}: rim cases covered: {counts} ({len(cloud)} planted gates)")
    assert cloud.misses == 0
    for case, n in need.items():
        assert counts[case] >= n, (name, case, counts)


def _check_rows(got, want, weighting, label):
    """The rule of test_gpu_roi_rim._check_csr on host arrays: (indptr, gate_indices, weights) against the oracle's"""
    ip, idx, w = oracle.canonical_rows(np.asarray(got[0], dtype=np.int64), np.asarray(got[1]), np.asarray(got[2], dtype=np.float32))
    o_ip, o_idx, o_w = want
    np.testing.assert_array_equal(ip, o_ip, err_msg=label)
    np.testing.assert_array_equal(idx, o_idx, err_msg=label)
    if weighting == "barnes2":
        assert np.abs(w.view(np.int32).astype(np.int64) - o_w.view(np.int32).astype(np.int64)).max(initial=0) <= 1, label
    else:
        np.testing.assert_array_equal(w.view(np.int32), o_w.view(np.int32), err_msg=label)
    return ip, idx, w


def _check_values(got, pairs, weighting, val, mask, report, label):
    """One gridded field [nz, n] (NaN fill) against the float64 oracle: NaN pattern, neighbours' range, the bound"""
    ip, idx, d2, r2 = pairs
    w64 = oracle.roi_weight_f64(d2, r2, weighting)
    n_rows = ip.shape[0] - 1
    want = oracle.csr_apply_f64(ip, idx, w64.astype(np.float32), val, mask, (n_rows,))
    _check_grid(got, want, ip, idx, val, mask, label)
    ratio = oracle.bound_ratio(got, oracle.voxel_stats(ip, idx, w64, val, mask), oracle.DELTA_K2[weighting])
    worst = float(ratio.max(initial=0.0))
    if report is not None:
        rec = REPORT.setdefault(report, {})
        rec[weighting] = max(rec.get(weighting, 0.0), worst)
    assert worst <= 1.0, (label, worst, int((ratio > 1).sum()))
    return worst


def _run(env, key, s, xs, ys, gates, pairs, weighting, fields, masks, variants, shared=None, report=None):
    """Checks 1 and 2 of the module docstring at the points (xs, ys) for every search variant"""
    rg, torch = env["rg"], env["torch"]
    ip, idx, d2, r2 = pairs
    assert idx.size > 0
    want_rows = (ip, idx, oracle.roi_weight_f64(d2, r2, weighting).astype(np.float32))
    merged = [m | shared if shared is not None else m for m in masks]
    f_t = [_dev(env, v) for v in fields]
    m_t = [_dev(env, m.astype(np.uint8), torch.uint8) for m in masks]
    s_t = None if shared is None else _dev(env, shared.astype(np.uint8), torch.uint8)
    nz, n = s.nz, len(xs)
    worst = 0.0
    for variant in variants:
        label = f"{key} {weighting} {SEARCHES[variant]}"
        search = _search(env, key, s, gates, variant)
        geom = rg.compute_section_geometry(search, xs, ys, weighting)
        assert geom.grid_shape == (nz, 1, n)
        _check_rows((geom.indptr, geom.gate_indices, geom.weights), want_rows, weighting, label)
        out = rg.section_fields_device(search, xs, ys, f_t, m_t, shared_mask=s_t, weighting=weighting).cpu().numpy()
        assert out.shape == (len(fields), nz, n)
        for k, (v, m) in enumerate(zip(fields, merged)):
            worst = max(worst, _check_values(out[k], pairs, weighting, v, m, report, f"{label} field {k}"))
    print(f"{key} {weighting}: worst err / bound {worst:.4f}")
    return search


def _gates(cloud):
    return cloud.gx, cloud.gy, cloud.gz


# ---- 1. the scenes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("name", srs.MAIN)
def test_rim_scenes(env, name, weighting):
    """Only planted rim gates, one field with some planted gates masked; per-level lists or one list, default or tiny cells
    (cell_size is clamped to span / 4000: cell boundaries everywhere along the rims)."""
    s, cloud = srs.scene(name), srs.cloud(name)
    _assert_coverage(name)
    own = srs.own_membership(name)
    assert own[np.isin(cloud.case, ["A", "B"])].all() and not own[np.isin(cloud.case, ["C", "D"])].any()
    val, mask = _values_and_mask(cloud.voxel, len(cloud), seed=3)
    if name in ("sparse_minr", "scattered"):      # samples whose only live neighbour has a float32 Cressman weight <= 0
        assert srs.a_only_samples(name, mask) >= 10
    _run(env, name, s, s.xs, s.ys, _gates(cloud), srs.pairs(name), weighting, [val], [mask], range(4), report=name)
    if name in ("sparse_minr", "scattered"):      # tiny cells: a block's box covers more than 64 cell rows (several rb trips)
        full = s.n // srs.KPTS
        for variant in (2, 3):
            cell = _SEARCH_CACHE[name, variant].cell_size
            assert srs.block_cell_rows(s, cell)[:full].min() > 64, (variant, cell)
    if name == "duplicates":                       # repeated points give identical rows, weights bit for bit
        geom = env["rg"].compute_section_geometry(_SEARCH_CACHE[name, 0], s.xs, s.ys, weighting)
        ip, idx, w = oracle.canonical_rows(geom.indptr, geom.gate_indices, geom.weights)
        for group in srs.DUPLICATE_GROUPS:
            for k in range(s.nz):
                first = k * s.n + group[0]
                assert ip[first + 1] > ip[first]
                for i in group[1:]:
                    r = k * s.n + i
                    np.testing.assert_array_equal(idx[ip[r]:ip[r + 1]], idx[ip[first]:ip[first + 1]])
                    np.testing.assert_array_equal(w[ip[r]:ip[r + 1]].view(np.int32), w[ip[first]:ip[first + 1]].view(np.int32))


@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("n_fields", [2, 3, 5])
def test_rim_scene_multi_field(env, n_fields, weighting):
    """2 / 3 / 5 fields (packed strides 2, 4 and 8) with per-field masks and a shared mask on sparse_minr"""
    name = "sparse_minr"
    s, cloud = srs.scene(name), srs.cloud(name)
    fields, masks = [], []
    for k in range(n_fields):
        v, m = _values_and_mask(cloud.voxel, len(cloud), seed=31 + k)
        fields.append(v); masks.append(m)
    shared = np.random.default_rng(37).random(len(cloud)) < 0.1
    _run(env, name, s, s.xs, s.ys, _gates(cloud), srs.pairs(name), weighting, fields, masks, range(2), shared=shared,
         report=name)


# ---- 2. rims in a dense background ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("name", srs.DENSE)
def test_rim_scenes_in_a_dense_background(env, name, weighting):
    """The planted gates anywhere in the index order among 30 000 random gates around the path: rows of 450 to 650
    neighbours pass through the 128-entry ring several times, and the rim gates share drains with ordinary ones."""
    s, cloud = srs.scene(name), srs.cloud(name)
    gx, gy, gz, where = srs.with_background(name)
    pairs = srs.background_pairs(name)
    assert np.diff(pairs[0]).max() > 256
    planted = np.full(gx.size, -1, dtype=np.int64)
    planted[where] = cloud.voxel
    # _values_and_mask masks one planted gate in some samples: give it the planted gates first, then permute as the gates are
    val0, mask0 = _values_and_mask(cloud.voxel, gx.size, seed=5)
    order = np.concatenate([where, np.setdiff1d(np.arange(gx.size), where)])
    val, mask = np.empty_like(val0), np.empty_like(mask0)
    val[order], mask[order] = val0, mask0
    np.testing.assert_array_equal(gx[where], cloud.gx)
    # the planted gates are still decided as labelled
    member = srs.membership(pairs[0], pairs[1], gx.size)[cloud.voxel, where]
    assert member[np.isin(cloud.case, ["A", "B"])].all() and not member[np.isin(cloud.case, ["C", "D"])].any()
    _run(env, name + "_bg", s, s.xs, s.ys, (gx, gy, gz), pairs, weighting, [val], [mask], range(3), report=name + "_bg")


# ---- 3. tails ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("n_points", [1, 2, 3, 4, 5])
def test_tails(env, n_points, weighting):
    """The first 1, 2, 3, 4 and 5 points of sparse_minr: one ragged block, one full block, a full and a ragged one"""
    name = "sparse_minr"
    s, cloud = srs.scene(name), srs.cloud(name)
    xs, ys = s.xs[:n_points].copy(), s.ys[:n_points].copy()
    pairs = sc.brute_pairs(cloud.gx, cloud.gy, cloud.gz, xs, ys, s.zc, radar_altitude=0.0, **s.roi)
    assert np.all(np.diff(pairs[0]).reshape(s.nz, n_points).sum(axis=0) > 0)
    val, mask = _values_and_mask(cloud.voxel, len(cloud), seed=3)
    _run(env, name, s, xs, ys, _gates(cloud), pairs, weighting, [val], [mask], range(4))


# ---- 4. dead lanes, through the C ABI ------------------------------------------------------------------------------------------------
BAD = (np.nan, np.inf, -np.inf)
PAD = 64
CANARY_I, CANARY_F = -123456789, -3.25e7


def _section_head(native, search, xs_t, ys_t, n):
    return (native.ptr(search.sorted_gates), native.ptr(search.cell_start), search.cells, native.ptr(xs_t), native.ptr(ys_t),
            native.ptr(search.zc), search.grid_shape[0], n, search.min_radius, search.beam_factor)


def _c_abi_section(env, search, xs, ys, weighting, val, mask):
    """rg_section_count_f32, rg_section_fill_f32 and rg_roi_section_f32 at points the Python surface would refuse, every
    output between canaries: (counts [rows], gate_indices, weights, grid [rows] with FILL)"""
    torch, native = env["torch"], env["native"]
    from radar_processor_amd.roi_grid import pack_and_grid
    lib = native.load_library()
    dev = env["dev"]
    nz, n = search.grid_shape[0], len(xs)
    n_rows = nz * n
    xs_t, ys_t = _dev(env, xs), _dev(env, ys)
    head = _section_head(native, search, xs_t, ys_t, n)
    with torch.cuda.device(dev):
        stream = native.stream_ptr()
        counts_buf = torch.full((PAD + n_rows + PAD,), CANARY_I, dtype=torch.int32, device=dev)
        assert lib.rg_section_count_f32(*head, native.ptr(counts_buf[PAD:]), stream) == native.RG_OK
        counts_all = counts_buf.cpu().numpy()
        assert np.all(counts_all[:PAD] == CANARY_I) and np.all(counts_all[PAD + n_rows:] == CANARY_I)
        counts = counts_all[PAD:PAD + n_rows].astype(np.int64)
        assert np.all(counts >= 0)
        indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        total = int(indptr[-1])
        gidx_buf = torch.full((PAD + total + PAD,), CANARY_I, dtype=torch.int32, device=dev)
        w_buf = torch.full((PAD + total + PAD,), CANARY_F, dtype=torch.float32, device=dev)
        indptr_t = torch.from_numpy(indptr).to(dev)
        assert lib.rg_section_fill_f32(*head, native.WEIGHTINGS[weighting], native.ptr(indptr_t), native.ptr(gidx_buf[PAD:]),
                                       native.ptr(w_buf[PAD:]), stream) == native.RG_OK
        gidx_all, w_all = gidx_buf.cpu().numpy(), w_buf.cpu().numpy()
        for a, canary in ((gidx_all, CANARY_I), (w_all, np.float32(CANARY_F))):
            assert np.all(a[:PAD] == canary) and np.all(a[PAD + total:] == canary)
        assert not np.any(gidx_all[PAD:PAD + total] == CANARY_I)           # every counted position was filled
        out_buf = torch.full((PAD + n_rows + PAD,), CANARY_F, dtype=torch.float32, device=dev)

        def launch(packed, nf, stride, out_view, stream_):
            assert lib.rg_roi_section_f32(*head, native.WEIGHTINGS[weighting], native.ptr(packed), nf, stride, FILL,
                                          native.ptr(out_view), stream_) == native.RG_OK
        pack_and_grid(dev, search.n_gates, [_dev(env, val)], [_dev(env, mask.astype(np.uint8), torch.uint8)], None,
                      out_buf[PAD:PAD + n_rows], (nz, n), launch)
        out_all = out_buf.cpu().numpy()
        assert np.all(out_all[:PAD] == np.float32(CANARY_F)) and np.all(out_all[PAD + n_rows:] == np.float32(CANARY_F))
    return counts, indptr, gidx_all[PAD:PAD + total], w_all[PAD:PAD + total], out_all[PAD:PAD + n_rows]


@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("name", srs.DENSE)
def test_dead_lanes_through_the_c_abi(env, name, weighting):
    """64 points cycling the path; block b = 0 .. 15 has live mask b, a dead point has NaN, +Inf or -Inf in x, in y or in
    both.  Dead rows: count 0 and the fill value.  Live rows: the oracle's rows of those points, values within the bound.
    (dense_minr: one radius for all; dense_beam: a radius that would be infinite for an infinite coordinate.)"""
    s, cloud = srs.scene(name), srs.cloud(name)
    n = 64
    pick = np.arange(n) % s.n
    xs, ys = s.xs[pick].copy(), s.ys[pick].copy()
    live = np.array([(b >> p) & 1 == 1 for b in range(16) for p in range(srs.KPTS)])
    kinds = set()
    for j, i in enumerate(np.nonzero(~live)[0]):
        bad, where = BAD[j % 3], (j // 3) % 3                               # where: 0 = x, 1 = y, 2 = both
        kinds.add((j % 3, where))
        if where in (0, 2):
            xs[i] = bad
        if where in (1, 2):
            ys[i] = bad
    assert len(kinds) == 9 and live.sum() == 32
    with pytest.raises(ValueError, match="finite"):
        env["rg"].compute_section_geometry(_search(env, name, s, _gates(cloud), 0), xs, ys, weighting)
    lx, ly = xs[live], ys[live]
    m = int(live.sum())
    lp = sc.brute_pairs(cloud.gx, cloud.gy, cloud.gz, lx, ly, s.zc, radar_altitude=0.0, **s.roi)
    # the oracle's rows over all 64 points: a dead point's rows are empty
    lengths = np.zeros((s.nz, n), dtype=np.int64)
    lengths[:, live] = np.diff(lp[0]).reshape(s.nz, m)
    assert lengths[:, live].min() > 0
    o_ip = np.concatenate([[0], np.cumsum(lengths.ravel())]).astype(np.int64)
    pairs = (o_ip, lp[1], lp[2], lp[3])              # row-major over (level, live point): the same order with the gaps
    want_rows = (o_ip, lp[1], oracle.roi_weight_f64(lp[2], lp[3], weighting).astype(np.float32))
    val, mask = _values_and_mask(cloud.voxel, len(cloud), seed=3)
    for variant in (0, 2):
        search = _search(env, name, s, _gates(cloud), variant)
        counts, ip, gidx, w, out = _c_abi_section(env, search, xs, ys, weighting, val, mask)
        label = f"{name} {weighting} {SEARCHES[variant]}"
        dead_rows = np.tile(~live, s.nz)
        assert np.all(counts[dead_rows] == 0), label
        assert np.all(out[dead_rows] == np.float32(FILL)), label
        _check_rows((ip, gidx, w), want_rows, weighting, label)
        got = out.astype(np.float32).copy()
        assert not np.isnan(got).any()
        got[got == np.float32(FILL)] = np.nan
        _check_values(got, pairs, weighting, val, mask, name + "_dead", label)


@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_a_section_of_dead_points_only(env, weighting):
    """Every point NaN: RG_OK, all counts 0, all fill (7 points: a full block and a ragged one)"""
    name = "dense_minr"
    s, cloud = srs.scene(name), srs.cloud(name)
    xs = np.full(7, np.nan, dtype=np.float32)
    val, mask = _values_and_mask(cloud.voxel, len(cloud), seed=3)
    for variant in (0, 2):
        counts, ip, gidx, w, out = _c_abi_section(env, _search(env, name, s, _gates(cloud), variant), xs, xs.copy(), weighting,
                                                  val, mask)
        assert counts.shape == (s.nz * 7,) and np.all(counts == 0) and gidx.size == 0
        assert np.all(out == np.float32(FILL))


# ---- 5. edges and windows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("name", srs.EDGES)
def test_points_on_the_rectangle_of_the_search(env, name, weighting):
    """Points on the corners and edge midpoints of the whole grid's rectangle and of a window's, their rim gates in the
    strip the cell grid pads by r_max only; (0, 0) with gates straight above and below, just inside and just outside."""
    s, cloud = srs.scene(name), srs.cloud(name)
    _assert_coverage(name)
    val, mask = _values_and_mask(cloud.voxel, len(cloud), seed=17)
    mask[len(cloud) - srs.n_vertical(name):] = False
    search = _run(env, name, s, s.xs, s.ys, _gates(cloud), srs.pairs(name), weighting, [val], [mask], range(4), report=name)
    assert env["rg"].section_rectangle(search) == srs.edge_rectangle(name.split("_")[1])
    assert (search.window != (0, s.grid_shape[1], 0, s.grid_shape[2])) == (s.window is not None)


# ---- 6. a rim cloud in a shifted frame, in a mosaic section -----------------------------------------------------------------------
RIM_ORIGIN = (317.25, 1234.5, -2718.75)          # oz != 0, horizontal offsets that are no multiples of the point spacing
ORDINARY = (ms.RadarSpec(seed=71, max_range_m=20e3, origin=(0.0, -4.1e3, -30.2e3)),
            ms.RadarSpec(seed=72, max_range_m=20e3, origin=(600.0, 3.3e3, 8.9e3)))
MOSAIC_NEED = dict(A=28, B=33, C=10, E=28)       # about half of what seed 9 yields


@functools.lru_cache(maxsize=1)
def _mosaic_scene():
    """sparse_minr's points and levels in the shared frame; the rim radar (table position 1, between two ordinary radars
    of mosaic_scenes) has as its gates a cloud planted around the points IN ITS OWN FRAME."""
    import radar_processor_amd as rg
    s = srs.scene("sparse_minr")
    limits = s.grid_limits
    x_r, y_r = mss.frame(s.xs, RIM_ORIGIN[2]), mss.frame(s.ys, RIM_ORIGIN[1])
    zc_r = oracle.axis_coords_f32(*rg.mosaic_limits(limits, RIM_ORIGIN)[0], s.nz)
    cloud = roi_rim.point_cloud(x_r, y_r, zc_r, s.min_radius, s.beam_factor, seed=9)
    vols = [ms.volume(spec) for spec in ORDINARY]
    radars = [(vols[0].gate_x, vols[0].gate_y, vols[0].gate_z, ORDINARY[0].origin), (cloud.gx, cloud.gy, cloud.gz, RIM_ORIGIN),
              (vols[1].gate_x, vols[1].gate_y, vols[1].gate_z, ORDINARY[1].origin)]
    pairs = []
    for gx, gy, gz, o in radars:
        pairs.append(sc.brute_pairs(gx, gy, gz, mss.frame(s.xs, o[2]), mss.frame(s.ys, o[1]),
                                    oracle.axis_coords_f32(*rg.mosaic_limits(limits, o)[0], s.nz), radar_altitude=0.0,
                                    min_radius=s.min_radius, beam_factor=s.beam_factor, toa=srs.TOA - o[0]))
    return s, cloud, vols, radars, pairs


@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_rim_cloud_in_a_shifted_frame_in_a_mosaic_section(env, weighting):
    rg, torch = env["rg"], env["torch"]
    s, cloud, vols, radars, pairs = _mosaic_scene()
    counts = cloud.counts()
    print(f"mosaic: rim cases covered: {counts} ({len(cloud)} planted gates)")
    assert cloud.misses == 0
    for case, n in MOSAIC_NEED.items():
        assert counts[case] >= n, (case, counts)
    n_rows = s.nz * s.n
    member = srs.membership(pairs[1][0], pairs[1][1], len(cloud))[cloud.voxel, np.arange(len(cloud))]
    assert member[np.isin(cloud.case, ["A", "B"])].all() and not member[cloud.case == "C"].any()
    reached = [np.diff(p[0]) > 0 for p in pairs]
    assert all(r.sum() >= 5 for r in reached) and int((reached[1] & (reached[0] | reached[2])).sum()) >= 3

    # the geometry route: every radar's part of every row is brute_pairs in that radar's frame
    geom = rg.compute_mosaic_section_geometry(radars, s.xs, s.ys, s.z_limits, s.nz, min_radius=s.min_radius,
                                              beam_factor=s.beam_factor, weighting=weighting, toa=srs.TOA)
    offsets = geom.gate_offsets
    for r, (ip, idx, d2, r2) in enumerate(pairs):
        seg = _segments(np.asarray(geom.indptr, dtype=np.int64), geom.gate_indices, geom.weights, offsets, r)
        _check_rows(seg, (ip, idx, oracle.roi_weight_f64(d2, r2, weighting).astype(np.float32)), weighting, f"radar {r}")

    # the CSR-free route, lattice windows and path searches: NaN pattern and bound against the float64 joint mean
    val, mask = _values_and_mask(cloud.voxel, len(cloud), seed=43)
    host = [oracle.merge_masks(vols[0].fields["DBZH"]), (val, mask), oracle.merge_masks(vols[1].fields["DBZH"])]
    j_ip, j_idx, j_w = ms.concat_rows([(p[0], p[1], oracle.roi_weight_f64(p[2], p[3], weighting)) for p in pairs],
                                      np.concatenate([[0], np.cumsum([len(r[0]) for r in radars])]))
    data = np.concatenate([h[0] for h in host]).astype(np.float32)
    excluded = np.concatenate([h[1] for h in host])
    stats = oracle.voxel_stats(j_ip, j_idx, j_w, data, excluded)
    assert np.isfinite(stats["m"]).sum() >= 80
    fields = [[_dev(env, h[0])] for h in host]
    masks = [[_dev(env, h[1].astype(np.uint8), torch.uint8)] for h in host]
    kw = dict(min_radius=s.min_radius, beam_factor=s.beam_factor, toa=srs.TOA)
    searches = {"lattice": rg.MosaicSearch(radars, s.grid_shape, s.grid_limits, **kw),
                "path": rg.MosaicSearch.for_path(radars, s.xs, s.ys, s.z_limits, s.nz, **kw)}
    for kind, search in searches.items():
        assert all(x is not None for x in search.searches)
        got = rg.mosaic_section_fields_device(search, s.xs, s.ys, fields, masks, weighting=weighting, combine="mean")
        got = got[0].cpu().numpy().ravel()
        assert got.shape == (n_rows,)
        ratio = oracle.bound_ratio(got, stats, oracle.DELTA_K2[weighting])        # +inf where the NaN patterns differ
        worst = float(ratio.max(initial=0.0))
        print(f"mosaic {kind} {weighting}: worst err / bound {worst:.4f}")
        rec = REPORT.setdefault("mosaic", {})
        rec[weighting] = max(rec.get(weighting, 0.0), worst)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(stats["m"]), err_msg=kind)
        assert worst <= 1.0, (kind, worst, int((ratio > 1).sum()))
