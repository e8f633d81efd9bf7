"""The mosaic combine rules on the MI355X (rg_roi_grid_mosaic_combine_f32 behind ``mosaic_fields_device(combine=...)``), on
``mosaic_scenes.scene16()`` (5 x 25 x 37, 16 radars) and the tie scene of tests/combine_scenes.py (3 x 9 x 21, 5 radars).

The yardstick needs no tolerance: a radar's own mean is what the existing mean path returns for that radar alone
(``radars=[r]``), so ``combine="max"`` / ``"nearest_radar"`` must equal, bit for bit, the NumPy fold (combine_scenes.fold) of
those per-radar grids, and ``return_radar`` the fold's winner on every voxel.  An independent check against the oracle's
float64 per-radar means (no code of the device path) bounds the values and pins the nearest radar."""
import numpy as np
import pytest

import combine_scenes as cs
from oracle import radar_grid_oracle as oracle

pytestmark = pytest.mark.gpu

WEIGHTINGS = ("barnes2", "cressman", "nearest")
FILL = cs.FILL


@pytest.fixture(scope="module")
def env():
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native
    rg.load_library()
    return dict(torch=torch, rg=rg, native=_native, dev=torch.device("cuda", 0), cache={})


def _dev(env, a, dtype=None):
    torch = env["torch"]
    return torch.from_numpy(np.ascontiguousarray(a)).to(env["dev"], dtype=dtype or torch.float32)


def _search(env, scene):
    key = ("search", scene.name)
    if key not in env["cache"]:
        env["cache"][key] = env["rg"].MosaicSearch(scene.radars(), scene.shape, scene.limits, min_radius=scene.min_radius,
                                                   beam_factor=scene.beam_factor, toa=scene.toa)
    return env["cache"][key]


def _call(env, fs, shared, sel, masked=True):
    """(fields, masks, shared_masks) of the radars ``sel`` on the device; ``masked=False``: no mask tensors at all."""
    torch = env["torch"]
    fields = [[_dev(env, d) for d, _ in fs[r]] for r in sel]
    if not masked:
        return fields, None, None
    masks = [[_dev(env, m.astype(np.uint8), torch.uint8) for _, m in fs[r]] for r in sel]
    return fields, masks, [_dev(env, shared[r].astype(np.uint8), torch.uint8) for r in sel]


def _per_radar(env, scene, fs, shared, weighting, masked, sel=None):
    """The existing mean path once per radar: ``(values float32 [R, F, V], has bool [R, F, V])`` in the order of ``sel``.  A
    radar without gates is not launched: it has no value anywhere."""
    rg = env["rg"]
    search = _search(env, scene)
    sel = list(range(scene.n_radars)) if sel is None else list(sel)
    nf = len(fs[0])
    n_vox = int(np.prod(scene.shape))
    values = np.full((len(sel), nf, n_vox), np.float32(FILL))
    for k, r in enumerate(sel):
        if len(scene.vols[r].gate_x) == 0:
            continue
        got = rg.mosaic_fields_device(search, *_call(env, fs, shared, [r], masked), weighting=weighting, fill_value=FILL,
                                      radars=[r])
        values[k] = got.cpu().numpy().reshape(nf, n_vox)
    return values, values != np.float32(FILL)


def _lattice_d(scene, sel=None):
    sel = range(scene.n_radars) if sel is None else sel
    return np.stack([cs.lattice_d(scene, r).ravel() for r in sel])


def _expect(values, has, d, combine, fill=FILL):
    """The fold, field by field: (out [F, V], who [F, V])."""
    folds = [cs.fold(values[:, f], has[:, f], combine, d, fill) for f in range(values.shape[1])]
    return np.stack([o for o, _ in folds]), np.stack([w for _, w in folds])


def _same_bits(got, want, label):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    np.testing.assert_array_equal(got.reshape(want.shape).view(np.int32), want.view(np.int32), err_msg=label)


def _same_radar(got, want, label):
    got = got.cpu().numpy()
    assert got.dtype == np.uint8
    np.testing.assert_array_equal(got.reshape(want.shape), want, err_msg=label)


# ---- 1. the fold of the per-radar grids, bit for bit --------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [1, 2, 3, 8])               # value-packed ring, stride-2 ring, gather per hit, the widest
@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("name", ["scene16", "tie"])
def test_combine_is_the_fold_of_the_per_radar_grids(env, name, weighting, nf):
    rg = env["rg"]
    scene = cs.scene(name)
    search = _search(env, scene)
    d = _lattice_d(scene)
    everyone = list(range(scene.n_radars))
    for masked in (True, False):
        fs, shared = cs.field_set(scene, nf, masked)
        values, has = _per_radar(env, scene, fs, shared, weighting, masked)
        assert has.any(axis=0).sum() > 100 * nf and (~has.any(axis=0)).sum() > 100 * nf       # filled and unfilled voxels
        assert (has.sum(axis=0) >= 2).sum() > 50 * nf                                        # ... and contested ones
        for combine in cs.COMBINES:
            label = f"{name} {weighting} {nf} field(s) masked={masked} {combine}"
            want, who = _expect(values, has, d, combine)
            got, radar = rg.mosaic_fields_device(search, *_call(env, fs, shared, everyone, masked), weighting=weighting,
                                                 fill_value=FILL, combine=combine, return_radar=True)
            assert tuple(got.shape) == (nf,) + scene.shape == tuple(radar.shape)
            _same_bits(got, want, label)
            _same_radar(radar, who, label)
            if combine == "max" and nf == 3:                                                 # without the provenance output
                alone = rg.mosaic_fields_device(search, *_call(env, fs, shared, everyone, masked), weighting=weighting,
                                                fill_value=FILL, combine=combine)
                _same_bits(alone, want, label + " (no radar map)")
        if name == "tie":           # the poison: a NaN held by slot 0 yields to a later number under max; an Inf wins
            vmax, wmax = _expect(values, has, d, "max")
            nan0 = np.isnan(values[0, 0]) & has[0, 0]
            assert nan0.any() and (wmax[0][nan0] != 0).any() and np.isposinf(vmax[0]).any()


def test_more_than_eight_fields_go_in_groups(env):
    rg = env["rg"]
    scene = cs.tie_scene()
    fs, shared = cs.field_set(scene, 10)
    values, has = _per_radar(env, scene, fs, shared, "cressman", True)
    want, who = _expect(values, has, _lattice_d(scene), "nearest_radar")
    got, radar = rg.mosaic_fields_device(_search(env, scene), *_call(env, fs, shared, range(scene.n_radars)),
                                         weighting="cressman", fill_value=FILL, combine="nearest_radar", return_radar=True)
    _same_bits(got, want, "10 fields")
    _same_radar(radar, who, "10 fields")


# ---- 2. the mean through the new entry point ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["scene16", "tie"])
def test_mean_through_the_new_entry_point_is_the_old_entry_point(env, name):
    torch, native = env["torch"], env["native"]
    from radar_processor_amd.mosaic import _concat_on_device, _offsets
    from radar_processor_amd.roi_grid import pack_and_grid
    lib = native.load_library()
    scene = cs.scene(name)
    search = _search(env, scene)
    nz, ny, nx = scene.shape
    sel = list(range(scene.n_radars))
    counts = [search.n_gates[r] for r in sel]
    table = search.table(sel, _offsets(counts)[:-1])
    n_total = sum(counts)
    for weighting in WEIGHTINGS:
        for nf in (1, 2, 3, 8):
            fs, shared = cs.field_set(scene, nf)
            fields, masks, shared_t = _call(env, fs, shared, sel)
            cat = _concat_on_device(fields, masks, shared_t, counts, nf, torch, env["dev"])
            outs = []
            for which in ("old", "new"):
                def launch(packed, nf_, stride, out_view, stream):
                    head = (table, len(sel), nz, ny, nx, search.min_radius, search.beam_factor, native.WEIGHTINGS[weighting],
                            native.ptr(packed), nf_, stride, n_total, float("nan"), native.ptr(out_view))
                    if which == "old":
                        rc = lib.rg_roi_grid_mosaic_f32(*head, stream)
                    else:
                        rc = lib.rg_roi_grid_mosaic_combine_f32(*head, native.COMBINES["mean"], None, stream)
                    native.check(rc, which)
                outs.append(pack_and_grid(env["dev"], n_total, *cat, None, scene.shape, launch).cpu().numpy())
            assert np.isfinite(outs[0]).sum() > 100 * nf
            np.testing.assert_array_equal(outs[0].view(np.int32), outs[1].view(np.int32), err_msg=f"{weighting} {nf}")


# ---- 3. one radar, table order, subsets ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combine", cs.COMBINES)
def test_a_one_radar_table_is_its_mean(env, combine):
    rg = env["rg"]
    scene = cs.tie_scene()
    search = _search(env, scene)
    fs, shared = cs.field_set(scene, 3)
    for r in (cs.TIE_POISON, cs.TIE_MIRROR[0]):
        for fill in (np.nan, FILL):
            call = _call(env, fs, shared, [r])
            mean = rg.mosaic_fields_device(search, *call, weighting="barnes2", fill_value=fill, radars=[r])
            got, radar = rg.mosaic_fields_device(search, *call, weighting="barnes2", fill_value=fill, radars=[r],
                                                 combine=combine, return_radar=True)
            _same_bits(got, mean.cpu().numpy(), f"radar {r} fill {fill}")
            # in the search, radar r is index r; where it has no value the map says so
            values, has = _per_radar(env, scene, fs, shared, "barnes2", True, sel=[r])
            _same_radar(radar, np.where(has[0], np.uint8(r), np.uint8(255)), f"radar {r}")
            assert has.any() and not has.all()


@pytest.mark.parametrize("combine", cs.COMBINES)
@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_the_colocated_pair_in_both_table_orders(env, weighting, combine):
    """The twins tie in value and in distance on every voxel they reach: the earlier table position wins, whichever twin
    stands there, and the values do not change."""
    rg = env["rg"]
    scene = cs.tie_scene()
    search = _search(env, scene)
    a, b = cs.TIE_TWINS
    fs, shared = cs.field_set(scene, 2)
    outs = {}
    for sel in ([a, b], [b, a], [cs.TIE_MIRROR[0], a, b], [cs.TIE_MIRROR[0], b, a]):
        got, radar = rg.mosaic_fields_device(search, *_call(env, fs, shared, sel), weighting=weighting, fill_value=FILL,
                                             radars=sel, combine=combine, return_radar=True)
        outs[tuple(sel)] = (got.cpu().numpy(), radar.cpu().numpy())
    (v_ab, r_ab), (v_ba, r_ba) = outs[(a, b)], outs[(b, a)]
    np.testing.assert_array_equal(v_ab.view(np.int32), v_ba.view(np.int32))
    filled = v_ab != np.float32(FILL)
    assert filled.sum() > 50 and (r_ab[filled] == a).all() and (r_ba[filled] == b).all()
    assert (r_ab[~filled] == 255).all() and (r_ba[~filled] == 255).all()
    (v3_ab, r3_ab), (v3_ba, r3_ba) = outs[(cs.TIE_MIRROR[0], a, b)], outs[(cs.TIE_MIRROR[0], b, a)]
    np.testing.assert_array_equal(v3_ab.view(np.int32), v3_ba.view(np.int32))
    twins = np.isin(r3_ab, (a, b))
    assert twins.sum() > 20 and (r3_ab[twins] == a).all() and (r3_ba[twins] == b).all()
    np.testing.assert_array_equal(r3_ab[~twins], r3_ba[~twins])


def test_a_subset_maps_positions_back_to_search_indices(env):
    rg = env["rg"]
    scene = cs.scene("scene16")
    search = _search(env, scene)
    sel = [13, 2, 9, 7, 4, 15, 0, 6]                    # shuffled; 7 (all masked) and 0 (far) have no value anywhere
    fs, shared = cs.field_set(scene, 2)
    values, has = _per_radar(env, scene, fs, shared, "barnes2", True, sel=sel)
    d = _lattice_d(scene, sel)
    for combine in cs.COMBINES:
        want, who = _expect(values, has, d, combine)
        got, radar = rg.mosaic_fields_device(search, *_call(env, fs, shared, sel), weighting="barnes2", fill_value=FILL,
                                             radars=sel, combine=combine, return_radar=True)
        _same_bits(got, want, combine)
        lut = np.full(256, 255, dtype=np.uint8)
        lut[:len(sel)] = sel
        _same_radar(radar, lut[who], combine)
        seen = set(np.unique(radar.cpu().numpy()).tolist())
        assert seen <= set(sel) | {255} and len(seen - {255}) >= 4 and 7 not in seen and 0 not in seen


def test_products_work_on_the_combined_grids(env):
    rg = env["rg"]
    scene = cs.scene("scene16")
    search = _search(env, scene)
    fs, shared = cs.field_set(scene, 2)
    call = _call(env, fs, shared, range(scene.n_radars))
    grids = rg.mosaic_fields_device(search, *call, combine="max")
    planes, radar = rg.mosaic_fields_device(search, *call, combine="max", products=rg.PlaneProducts(colmax=True, argmax=False),
                                            return_radar=True)
    assert len(planes) == 2 and tuple(radar.shape) == (2,) + scene.shape
    want = np.fmax.reduce(np.where(np.isnan(grids.cpu().numpy()), -np.inf, grids.cpu().numpy()), axis=1)
    got = np.stack([p["colmax"].cpu().numpy() for p in planes])
    np.testing.assert_array_equal(np.where(np.isnan(got), -np.inf, got), want)


# ---- 4. against the oracle's float64 per-radar means --------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("name", ["scene16", "tie"])
def test_values_lie_within_the_bound_of_the_named_radars_float64_mean(env, name, weighting):
    """No code of the device path: per radar the oracle's CSR (Scene.csr, weights_f64) gives the float64 mean ``m_r`` and the
    live count ``n_r``.  Every filled voxel lies within oracle.mean_error_bound (DELTA_K2) of the mean of the radar the map
    names (where that mean is not finite -- the poison -- the value is the same NaN or infinity); a voxel is the fill exactly
    where no radar has a live neighbour; under nearest_radar the named radar is the argmin of the float64 D among the radars
    with a live neighbour, the earliest of equals."""
    rg = env["rg"]
    scene = cs.scene(name)
    search = _search(env, scene)
    nf = 3
    fs, shared = cs.field_set(scene, nf)
    d = _lattice_d(scene)
    stats = [[cs.radar_stats(scene, weighting, fs, shared, k, r) for r in range(scene.n_radars)] for k in range(nf)]
    for combine in cs.COMBINES:
        got, radar = rg.mosaic_fields_device(search, *_call(env, fs, shared, range(scene.n_radars)), weighting=weighting,
                                             fill_value=FILL, combine=combine, return_radar=True)
        got, radar = got.cpu().numpy().reshape(nf, -1), radar.cpu().numpy().reshape(nf, -1)
        for k in range(nf):
            n = np.stack([s["n"] for s in stats[k]])
            np.testing.assert_array_equal(radar[k] == 255, (n > 0).sum(axis=0) == 0)
            np.testing.assert_array_equal(got[k] == np.float32(FILL), radar[k] == 255)
            if combine == "nearest_radar":
                want = np.where((n > 0).any(axis=0), np.argmin(np.where(n > 0, d, np.inf), axis=0), 255)
                np.testing.assert_array_equal(radar[k], want.astype(np.uint8))
            checked = 0
            for r in range(scene.n_radars):
                at = radar[k] == r
                if not at.any():
                    continue
                sub = {key: np.asarray(v)[at] for key, v in stats[k][r].items()}
                fin = np.isfinite(sub["m"])
                ratio = oracle.bound_ratio(got[k][at][fin], {key: v[fin] for key, v in sub.items()}, oracle.DELTA_K2[weighting])
                assert ratio.max(initial=0.0) <= 1.0, (combine, k, r, float(ratio.max()))
                odd = got[k][at][~fin]                    # an Inf gives an infinite mean; a NaN (or Inf - Inf) a NaN
                assert np.all(np.isnan(odd) | (odd == sub["m"][~fin].astype(np.float32))) and not np.isfinite(odd).any()
                checked += int(fin.sum())
            assert checked > 250, checked
