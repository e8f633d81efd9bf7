"""Mosaics of 16 and 20 radars on the MI355X (the seeded scenes of tests/mosaic_scenes.py) against the float64 mosaic mean.

 1. Geometry route, 16 and 20 radars: ``compute_mosaic_geometry`` equals the row-wise concatenation of the oracle's CSRs
    (indptr, gate offsets, every radar's segment; Cressman / nearest weights bit for bit, Barnes within one ulp) -- the
    merge's running cursor with up to 20 segments per row.  Grids of 1, 2, 3, 5 and 8 fields through
    ``apply_mosaic_multi`` and ``mosaic_fields_device`` within ``bound_ratio <= 1`` (oracle.DELTA_CSR) of the float64 mean,
    NaN fill and -9999 fill; the row-wise kernel over the packed records for 1 and 8 fields.
 2. CSR-free route on ``scene16`` (the full table of RG_MAX_RADARS = 16 entries): every field count 1-8 through
    ``rg_roi_grid_mosaic_f32`` for all three weightings within oracle.DELTA_K2; slots 0, 7 and 15 read one by one against
    ``rg_roi_grid_f32``; radar order and subsets; inert radars; per-radar search structures of different kinds in one table.
 3. A rim cloud (oracle/roi_rim.py) planted in one radar's shifted frame, gridded in a mosaic with ordinary radars: its
    segment of the mosaic geometry is the oracle's CSR."""
import ctypes
import functools

import numpy as np
import pytest

import mosaic_scenes
from mosaic_scenes import FIELDS, MIN_RADIUS, TOA
from oracle import radar_grid_oracle as oracle
from oracle import roi_rim
from test_gpu_mosaic import _entry_of, _segments, _ulp

pytestmark = pytest.mark.gpu

WEIGHTINGS = ("barnes2", "cressman", "nearest")
SEARCHES = (dict(), dict(per_level=False), dict(per_level=True, cell_size=1.0), dict(per_level=False, cell_size=1.0))


@pytest.fixture(scope="module")
def env():
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native
    rg.load_library()
    return dict(torch=torch, rg=rg, native=_native, dev=torch.device("cuda", 0))


def _stride(nf):
    return 1 if nf == 1 else 2 if nf == 2 else 4 if nf <= 4 else 8


def _dev(env, a, dtype=None):
    torch = env["torch"]
    return torch.from_numpy(np.ascontiguousarray(a)).to(env["dev"], dtype=dtype or torch.float32)


# ---- field sets ---------------------------------------------------------------------------------------------------------------
def _field_set(scene, nf, seed, nan_radar=None):
    """Per radar: ``nf`` fields (value, field mask) -- field k is FIELDS[k % 3] of the radar plus k, its mask the field's own
    mask (all gates for the 'masked' radar) with 5 % more gates masked from field 3 on -- and one shared QC mask (RHOHV
    below 0.8).  ``nan_radar``: three NaN values of that radar's field 0 are left unmasked (they poison their voxels on both
    sides)."""
    rng = np.random.default_rng(seed)
    out, shared = [], []
    for r, v in enumerate(scene.vols):
        n = len(v.gate_x)
        qc = oracle.gate_mask("below", np.ma.getdata(v.fields["RHOHV"]), 0.8) if n else np.zeros(0, dtype=bool)
        fs = []
        for k in range(nf):
            f = v.fields[FIELDS[k % 3]]
            data = (np.ma.getdata(f) + np.float32(k)).astype(np.float32)
            mask = np.ma.getmaskarray(f).copy()
            if k >= 3:
                mask |= rng.random(n) < 0.05
            fs.append((data, mask))
        if r == nan_radar:                        # NaN gates that are neighbours of some voxel and pass the QC mask
            nan_at = np.nonzero(np.isnan(fs[0][0]) & ~qc)[0]
            nan_at = nan_at[np.isin(nan_at, scene.csr(r)[1])][:3]
            assert nan_at.size == 3
            fs[0][1][nan_at] = False
        out.append(fs)
        shared.append(qc)
    return out, shared


def _stats(scene, weighting, fs, shared, k, sel=None):
    """oracle.voxel_stats of field k over the radars ``sel`` (default: all), field mask | shared mask."""
    sel = list(range(scene.n_radars)) if sel is None else list(sel)
    ip, idx, w64 = scene.mosaic_csr(weighting, sel)
    data = np.concatenate([fs[r][k][0] for r in sel])
    mask = np.concatenate([fs[r][k][1] | shared[r] for r in sel])
    return oracle.voxel_stats(ip, idx, w64, data, mask)


def _assert_bound(got, stats, delta, label):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    ratio = oracle.bound_ratio(got, stats, delta)
    assert np.isfinite(stats["m"]).sum() > 500, label                      # the comparison is not vacuous
    assert ratio.max(initial=0.0) <= 1.0, (label, float(ratio.max()), int((ratio > 1).sum()))


def _device_call(env, scene, fs, shared, sel=None):
    torch = env["torch"]
    sel = list(range(scene.n_radars)) if sel is None else list(sel)
    fields = [[_dev(env, d) for d, _ in fs[r]] for r in sel]
    masks = [[_dev(env, m.astype(np.uint8), torch.uint8) for _, m in fs[r]] for r in sel]
    shared_t = [_dev(env, shared[r].astype(np.uint8), torch.uint8) for r in sel]
    return fields, masks, shared_t


# ---- 1. geometry route ----------------------------------------------------------------------------------------------------
_GEOMS = {}


def _geometry(env, name, weighting, tmp_path_factory):
    key = (name, weighting)
    if key not in _GEOMS:
        scene = getattr(mosaic_scenes, name)()
        _GEOMS[key] = env["rg"].compute_mosaic_geometry(scene.radars(), scene.shape, scene.limits,
                                                        str(tmp_path_factory.mktemp("mosaic")), min_radius=MIN_RADIUS,
                                                        weighting=weighting, toa=TOA)
    return _GEOMS[key]


@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("name", ["scene16", "scene20"])
def test_many_radar_geometry_matches_the_oracle(env, name, weighting, tmp_path_factory):
    """16 and 20 radars (20: more than one CSR-free launch takes) through compute_mosaic_geometry: the merge's indptr and
    gate offsets equal the oracle's concatenation, every radar's segment of every row holds the oracle's pairs."""
    scene = getattr(mosaic_scenes, name)()
    geom = _geometry(env, name, weighting, tmp_path_factory)
    offsets = scene.offsets()
    np.testing.assert_array_equal(geom.gate_offsets, offsets)
    ip, _, _ = scene.mosaic_csr(weighting, exact=False)
    np.testing.assert_array_equal(np.asarray(geom.indptr, dtype=np.int64), ip)
    row_len = np.diff(ip)
    assert (np.sum([np.diff(scene.csr(r)[0]) > 0 for r in range(scene.n_radars)], axis=0)).max() >= 8
    assert row_len.max() > 0 and geom.n_pairs() == int(ip[-1])
    for r in range(scene.n_radars):
        s_ip, s_idx, s_w = oracle.canonical_rows(*_segments(geom.indptr, geom.gate_indices, geom.weights, offsets, r))
        o_ip, o_idx, o_w = oracle.canonical_rows(scene.csr(r)[0], scene.csr(r)[1], scene.weights_f32(r, weighting))
        np.testing.assert_array_equal(s_ip, o_ip, err_msg=f"radar {r}")
        np.testing.assert_array_equal(s_idx, o_idx, err_msg=f"radar {r}")
        if weighting == "barnes2":
            assert _ulp(s_w, o_w).max(initial=0) <= 1, r
        else:
            np.testing.assert_array_equal(s_w.view(np.int32), o_w.view(np.int32), err_msg=f"radar {r}")


@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("name", ["scene16", "scene20"])
def test_many_radar_geometry_grids_within_the_bound(env, name, weighting, tmp_path_factory):
    """1, 2, 3, 5 and 8 fields through the mosaic geometry: apply_mosaic_multi (GateFilter lists on some radars, NaN fill
    and -9999 fill) and mosaic_fields_device (per-field masks, a shared mask, unmasked NaNs), within DELTA_CSR of the
    float64 mean; -9999 exactly where the oracle has no live neighbour."""
    rg = env["rg"]
    scene = getattr(mosaic_scenes, name)()
    geom = _geometry(env, name, weighting, tmp_path_factory)
    delta = oracle.DELTA_CSR[weighting]
    live = [r for r, k in enumerate(scene.kinds) if k == "live"]
    qc_radars = set(live[::3])                                     # a GateFilter list on every third live radar
    for nf in (1, 2, 3, 5, 8):
        fs, shared = _field_set(scene, nf, seed=nf)
        names = [f"f{k}" for k in range(nf)]
        fields = {names[k]: [np.ma.array(fs[r][k][0], mask=fs[r][k][1]) for r in range(scene.n_radars)]
                  for k in range(nf)}
        filters = []
        for r, v in enumerate(scene.vols):
            filters.append([rg.GateFilter(v.as_radar()).exclude_below("RHOHV", 0.8)] if r in qc_radars else [])
        with_qc = [shared[r] if r in qc_radars else np.zeros_like(shared[r]) for r in range(scene.n_radars)]
        for fill in (np.nan, -9999.0):
            grids = rg.apply_mosaic_multi(geom, fields, {n: filters for n in names}, fill_value=fill)
            for k, n in enumerate(names):
                stats = _stats(scene, weighting, fs, with_qc, k)
                got = grids[n].copy()
                if not np.isnan(fill):
                    empty = stats["n"].reshape(scene.shape) == 0
                    np.testing.assert_array_equal(got == np.float32(fill), empty, err_msg=f"{nf} fields, {n}")
                    got[empty] = np.nan
                _assert_bound(got, stats, delta, f"apply_mosaic_multi {nf} fields {n} fill {fill}")
        fs, shared = _field_set(scene, nf, seed=10 + nf, nan_radar=live[1])
        got = rg.mosaic_fields_device(geom, *_device_call(env, scene, fs, shared))
        for k in range(nf):
            stats = _stats(scene, weighting, fs, shared, k)
            if k == 0:
                assert np.isnan(stats["m"][stats["n"] > 0]).sum() >= 3           # the unmasked NaNs reach voxels
            _assert_bound(got[k], stats, delta, f"mosaic_fields_device {nf} fields, field {k}")


@pytest.mark.parametrize("weighting", ["barnes2", "nearest"])            # Cressman weights have no 26-bit code
@pytest.mark.parametrize("name", ["scene16", "scene20"])
def test_many_radar_rowwise_kernel_within_the_bound(env, name, weighting, tmp_path_factory):
    """The row-wise kernel over the packed records of the mosaic geometry's compact copy (forced, as in
    test_gpu_mean_bounds: on a geometry this small CsrGridder's own policy keeps the standard kernel), a 1-field pass (must
    stream the packed records) and an 8-field pass (if the records cannot be streamed, the standard kernel -- reported and
    bounded the same way)."""
    torch, dev = env["torch"], env["dev"]
    from radar_processor_amd.gridding import CsrGridder
    scene = getattr(mosaic_scenes, name)()
    geom = _geometry(env, name, weighting, tmp_path_factory)
    n_total = int(scene.offsets()[-1])
    compact = geom.device_compact(dev)
    for nf in (1, 8):
        fs, shared = _field_set(scene, nf, seed=20 + nf)
        gr = CsrGridder(geom, n_total, nf, device=dev)
        packed = compact.ensure_packed(gr.csr)
        if packed:
            gr.compact, gr.packed_stream = compact, True
            gr.window = compact.window_for(nf, rowwise=True)
        kernel = "row-wise" if gr.packed_stream else "standard"
        print(f"{name} {weighting} {nf} field(s): {kernel} kernel, LDS window {gr.window}, "
              f"{compact.fallback_fraction(gr.window):.3f} of the pairs gathered per pair")
        if nf == 1:
            assert gr.packed_stream, "a one-field pass over the compact copy streams the packed records"
        cat = [_dev(env, np.concatenate([fs[r][k][0] for r in range(scene.n_radars)])) for k in range(nf)]
        cat_m = [_dev(env, np.concatenate([fs[r][k][1] for r in range(scene.n_radars)]).astype(np.uint8), torch.uint8)
                 for k in range(nf)]
        gr.pack(cat, cat_m, _dev(env, np.concatenate(shared).astype(np.uint8), torch.uint8))
        out = torch.empty((nf, gr.n_vox), dtype=torch.float32, device=dev)
        gr.apply(out)
        for k in range(nf):
            _assert_bound(out[k], _stats(scene, weighting, fs, shared, k), oracle.DELTA_CSR[weighting],
                          f"{kernel} kernel, {nf} fields, field {k}")


# ---- 2. CSR-free route, 16 radars -----------------------------------------------------------------------------------------------
_SEARCH = {}


def _mosaic_search(env):
    if "scene16" not in _SEARCH:
        scene = mosaic_scenes.scene16()
        _SEARCH["scene16"] = env["rg"].MosaicSearch(scene.radars(), scene.shape, scene.limits, min_radius=MIN_RADIUS,
                                                    toa=TOA)
    return _SEARCH["scene16"]


@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_sixteen_radars_every_field_count(env, weighting):
    """The full table (slots 0-15, slot 15 live) through rg_roi_grid_mosaic_f32 for every field count 1-8 -- the value
    ring (1-2 fields, the value in the queued record for 1 weighted field), the strides 4 (3-4 fields) and 8 (5-8) --
    with per-field and shared masks, within DELTA_K2 of the float64 mean."""
    rg = env["rg"]
    scene = mosaic_scenes.scene16()
    ms = _mosaic_search(env)
    assert ms.n_radars == env["native"].RG_MAX_RADARS == 16
    assert ms.searches[0] is None and ms.searches[15] is not None and ms.searches[7] is not None
    for nf in range(1, 9):
        fs, shared = _field_set(scene, nf, seed=30 + nf)
        got = rg.mosaic_fields_device(ms, *_device_call(env, scene, fs, shared), weighting=weighting)
        assert got.shape == (nf,) + scene.shape
        for k in range(nf):
            _assert_bound(got[k], _stats(scene, weighting, fs, shared, k), oracle.DELTA_K2[weighting],
                          f"{nf} fields, field {k}")


def _pack(env, values, masks, nf):
    """rg_pack_fields_f32 of ``nf`` host fields (lists of float32 / bool arrays of one length) -> the packed buffer."""
    torch, native = env["torch"], env["native"]
    lib = native.load_library()
    n = len(values[0])
    vals = [_dev(env, v) for v in values]
    msks = [_dev(env, m.astype(np.uint8), torch.uint8) for m in masks]
    packed = torch.empty(max(n, 1) * _stride(nf), dtype=torch.float32, device=env["dev"])
    fp = (ctypes.c_void_p * nf)(*[native.ptr(v) for v in vals])
    mp = (ctypes.c_void_p * nf)(*[native.ptr(m) for m in msks])
    native.check(lib.rg_pack_fields_f32(nf, fp, mp, None, n, _stride(nf), native.ptr(packed), native.stream_ptr()), "pack")
    return packed


@pytest.mark.parametrize("slot", [0, 7, 15])
def test_each_slot_is_read(env, slot):
    """A 16-entry table whose only live entry, at ``slot``, is one radar's whole-grid search at a non-zero packed offset;
    the other 15 entries reach nothing but own gate ranges before and after it (filled with values that would show if
    they were read).  The result is the bits of rg_roi_grid_f32 for that radar alone, for 1, 2, 4 and 8 fields."""
    torch, rg, native = env["torch"], env["rg"], env["native"]
    lib = native.load_library()
    scene = mosaic_scenes.scene16()
    r = 6                                    # live; its neighbours reach the x-max and y-min faces of the grid
    v, o = scene.vols[r], scene.origins[r]
    nz, ny, nx = scene.shape
    s = rg.RoiSearch(v.gate_x, v.gate_y, v.gate_z, scene.shape, rg.mosaic_limits(scene.limits, o), min_radius=MIN_RADIUS,
                     toa=TOA - o[0])
    assert s.window == (0, ny, 0, nx)
    n = s.n_gates
    pads = [1000 + 37 * j for j in range(16)]                           # gates of the other entries
    offsets = np.concatenate([[0], np.cumsum([n if j == slot else pads[j] for j in range(16)])]).astype(np.int64)
    n_total = int(offsets[-1])
    lead = 4099                                      # a pad before the first entry: the radar never sits at offset 0
    rng = np.random.default_rng(slot)
    for weighting in WEIGHTINGS:
        for nf in (1, 2, 4, 8):
            vals = [(rng.random(n) * 70 - 10).astype(np.float32) for _ in range(nf)]
            msks = [rng.random(n) < 0.3 for _ in range(nf)]
            one = _pack(env, vals, msks, nf)
            a = torch.empty((nf, nz * ny * nx), dtype=torch.float32, device=env["dev"])
            native.check(lib.rg_roi_grid_f32(native.ptr(s.sorted_gates), native.ptr(s.cell_start), s.cells,
                                             native.ptr(s.xc), native.ptr(s.yc), native.ptr(s.zc), nz, ny, nx, s.min_radius,
                                             s.beam_factor, native.WEIGHTINGS[weighting], native.ptr(one), nf, _stride(nf),
                                             float("nan"), native.ptr(a), native.stream_ptr()), "rg_roi_grid_f32")
            # the shared buffer: lead pad, then the 16 entries' gate ranges; every pad value is live and far off the data
            big = [np.full(lead + n_total, 1e4 + 17 * f, dtype=np.float32) for f in range(nf)]
            big_m = [np.zeros(lead + n_total, dtype=bool) for _ in range(nf)]
            at = lead + int(offsets[slot])
            for f in range(nf):
                big[f][at:at + n] = vals[f]
                big_m[f][at:at + n] = msks[f]
            packed = _pack(env, big, big_m, nf)
            table = (native.MosaicRadar * 16)()
            for j in range(16):
                if j == slot:
                    table[j] = _entry_of(native, s, at)
                else:
                    table[j].gate_offset, table[j].n_gates = lead + int(offsets[j]), pads[j]
            b = torch.empty_like(a)
            native.check(lib.rg_roi_grid_mosaic_f32(table, 16, nz, ny, nx, s.min_radius, s.beam_factor,
                                                    native.WEIGHTINGS[weighting], native.ptr(packed), nf, _stride(nf),
                                                    lead + n_total, float("nan"), native.ptr(b), native.stream_ptr()),
                         "rg_roi_grid_mosaic_f32")
            assert torch.isfinite(a).sum() > 100
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"slot {slot}, {weighting}, {nf} fields"


def test_radar_order_subsets_and_inert_radars(env):
    """``radars=`` reversed, shuffled and a 9-radar subset: each within DELTA_K2 of the oracle's mean over that subset;
    dropping the four inert radars (far, no gates, all masked, above toa) from the call changes no bit."""
    rg = env["rg"]
    torch = env["torch"]
    scene = mosaic_scenes.scene16()
    ms = _mosaic_search(env)
    weighting = "barnes2"
    nf = 2
    fs, shared = _field_set(scene, nf, seed=40)
    rng = np.random.default_rng(41)
    orders = {"reversed": list(range(15, -1, -1)), "shuffled": [int(r) for r in rng.permutation(16)],
              "subset": sorted(int(r) for r in rng.choice(16, 9, replace=False))}
    for label, sel in orders.items():
        got = rg.mosaic_fields_device(ms, *_device_call(env, scene, fs, shared, sel), weighting=weighting, radars=sel)
        for k in range(nf):
            _assert_bound(got[k], _stats(scene, weighting, fs, shared, k, sel=sel), oracle.DELTA_K2[weighting],
                          f"{label} {sel}, field {k}")
    live = [r for r, kind in enumerate(scene.kinds) if kind == "live"]
    assert len(live) == 12
    full = rg.mosaic_fields_device(ms, *_device_call(env, scene, fs, shared), weighting=weighting)
    only_live = rg.mosaic_fields_device(ms, *_device_call(env, scene, fs, shared, live), weighting=weighting, radars=live)
    assert torch.equal(full.view(torch.int32), only_live.view(torch.int32))


@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_mixed_search_structures_in_one_table(env, weighting):
    """Per radar a RoiSearch over its reach window of a different kind -- per-level lists or one list, automatic or 1 m
    cells (clamped to the lattice limit) -- all in one 16-entry table: within DELTA_K2 of the float64 mean."""
    torch, rg, native = env["torch"], env["rg"], env["native"]
    lib = native.load_library()
    scene = mosaic_scenes.scene16()
    nz, ny, nx = scene.shape
    offsets = scene.offsets()
    searches, kinds = [], set()
    for r in range(scene.n_radars):
        v, o = scene.vols[r], scene.origins[r]
        w = scene.window(r)
        if w == (0, 0, 0, 0):
            searches.append(None)
            continue
        skw = SEARCHES[r % len(SEARCHES)]
        s = rg.RoiSearch(v.gate_x, v.gate_y, v.gate_z, scene.shape, rg.mosaic_limits(scene.limits, o),
                         min_radius=MIN_RADIUS, toa=TOA - o[0], window=w, **skw)
        if "per_level" in skw:
            assert s.per_level == skw["per_level"]
        kinds.add((s.per_level, "cell_size" in skw))
        searches.append(s)
    assert len(kinds) == 4
    table = (native.MosaicRadar * 16)()
    for r, s in enumerate(searches):
        if s is None:
            table[r].gate_offset, table[r].n_gates = int(offsets[r]), len(scene.vols[r].gate_x)
        else:
            table[r] = _entry_of(native, s, int(offsets[r]))
    for nf in (1, 3, 6):
        fs, shared = _field_set(scene, nf, seed=50 + nf)
        merged = [[fs[r][k][1] | shared[r] for r in range(16)] for k in range(nf)]
        packed = _pack(env, [np.concatenate([fs[r][k][0] for r in range(16)]) for k in range(nf)],
                       [np.concatenate(merged[k]) for k in range(nf)], nf)
        out = torch.empty((nf, nz * ny * nx), dtype=torch.float32, device=env["dev"])
        native.check(lib.rg_roi_grid_mosaic_f32(table, 16, nz, ny, nx, MIN_RADIUS, scene.beam_factor,
                                                native.WEIGHTINGS[weighting], native.ptr(packed), nf, _stride(nf),
                                                int(offsets[-1]), float("nan"), native.ptr(out), native.stream_ptr()),
                     "rg_roi_grid_mosaic_f32")
        for k in range(nf):
            _assert_bound(out[k], _stats(scene, weighting, fs, shared, k), oracle.DELTA_K2[weighting],
                          f"{nf} fields, field {k}")


# ---- 3. the rim in a shifted frame ------------------------------------------------------------------------------------------
RIM_SHAPE = (3, 9, 37)                  # 2.5 km apart in every direction: > 2 r_max (r = 1000 m)
RIM_LIMITS = ((500.0, 5500.0), (-10e3, 10e3), (-45e3, 45e3))
RIM_ORIGIN = (317.25, 1234.5, -2718.75)        # oz != 0, horizontal offsets that are not voxel multiples
RIM_NEED = dict(A=300, B=300, C=100, E=300)     # D needs integer voxels and radius: none here


@functools.lru_cache(maxsize=1)
def _rim_cloud():
    from radar_processor_amd.mosaic import mosaic_limits
    return roi_rim.rim_cloud(RIM_SHAPE, mosaic_limits(RIM_LIMITS, RIM_ORIGIN), 1000.0, 0.0, seed=3)


@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_rim_cloud_in_a_shifted_frame(env, weighting, tmp_path):
    """Gates planted at the rims of every voxel in the frame of a radar at RIM_ORIGIN (oracle.roi_rim on the shifted
    limits), in a mosaic with three ordinary radars: the rim radar's segment of the mosaic geometry is the oracle's CSR
    (Cressman / nearest bit for bit, Barnes within one ulp), and so is every other radar's."""
    rg = env["rg"]
    from radar_processor_amd import synthetic
    cloud = _rim_cloud()
    counts = cloud.counts()
    print(f"rim cases covered: {counts} ({len(cloud)} planted gates)")
    assert cloud.misses == 0
    for case, n in RIM_NEED.items():
        assert counts[case] >= n, (case, counts)
    vols = [synthetic.make_volume(n_elev=4, n_az=60, n_gates=40, seed=60 + k, max_range_m=20e3) for k in range(3)]
    radars = [(vols[0].gate_x, vols[0].gate_y, vols[0].gate_z, (0.0, -4.1e3, -30.2e3)),
              (cloud.gx, cloud.gy, cloud.gz, RIM_ORIGIN),
              (vols[1].gate_x, vols[1].gate_y, vols[1].gate_z, (600.0, 3.3e3, 8.9e3)),
              (vols[2].gate_x, vols[2].gate_y, vols[2].gate_z, (250.0, -7.7e3, 33.1e3))]
    geom = rg.compute_mosaic_geometry(radars, RIM_SHAPE, RIM_LIMITS, str(tmp_path), min_radius=1000.0, beam_factor=0.0,
                                      weighting=weighting, toa=17000.0)
    offsets = geom.gate_offsets
    csrs = []
    for r, (gx, gy, gz, o) in enumerate(radars):
        o_ip, o_idx, o_w = oracle.build_geometry(gx, gy, gz, RIM_SHAPE, rg.mosaic_limits(RIM_LIMITS, o), min_radius=1000.0,
                                                 beam_factor=0.0, weighting=weighting, toa=17000.0 - o[0])
        assert o_ip[-1] > 0
        csrs.append((o_ip, o_idx, o_w))
        s_ip, s_idx, s_w = oracle.canonical_rows(*_segments(geom.indptr, geom.gate_indices, geom.weights, offsets, r))
        np.testing.assert_array_equal(s_ip, o_ip, err_msg=f"radar {r}")
        np.testing.assert_array_equal(s_idx, o_idx, err_msg=f"radar {r}")
        if weighting == "barnes2":
            assert _ulp(s_w, o_w).max(initial=0) <= 1, r
        else:
            np.testing.assert_array_equal(s_w.view(np.int32), o_w.view(np.int32), err_msg=f"radar {r}")
    # the planted labels are what the oracle sees: A / B inside, C outside
    o_ip, o_idx, _ = csrs[1]
    row = np.repeat(np.arange(o_ip.shape[0] - 1), np.diff(o_ip))
    member = set(zip(row.tolist(), o_idx.tolist()))
    pair_in = np.array([(int(v), i) in member for i, v in enumerate(cloud.voxel)])
    assert pair_in[np.isin(cloud.case, ["A", "B"])].all() and not pair_in[cloud.case == "C"].any()
