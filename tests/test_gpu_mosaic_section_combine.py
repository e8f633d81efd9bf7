"""The mosaic combine rules on a vertical section, on the MI355X (rg_roi_section_mosaic_combine_f32 behind
``mosaic_section_fields_device(combine=...)``): a dog-leg of 91 points through ``mosaic_scenes.scene16()`` and 23 points
through the tie scene of tests/combine_scenes.py, eight of them exactly on the mirror column -- 4k + 3 points each, so the
section kernel's last block of a level is ragged.

As in tests/test_gpu_mosaic_combine.py the yardstick is exact: the NumPy fold (combine_scenes.fold) of the per-radar
sections ``mosaic_section_fields_device(radars=[r])`` of the existing mean path, bit for bit, and its winner as the radar
map; then the mean through the new entry point, one radar alone, the co-located pair in both orders, a subset, and the
oracle's float64 per-radar means of the brute-force neighbours."""
import numpy as np
import pytest

import combine_scenes as cs
from oracle import radar_grid_oracle as oracle
from test_gpu_mosaic_combine import FILL, WEIGHTINGS, _call, _expect, _same_bits, _same_radar, _search, env  # noqa: F401

pytestmark = pytest.mark.gpu


def _per_radar(env, scene, xs, ys, fs, shared, weighting, sel=None):
    """The existing mean path once per radar: ``(values float32 [R, F, S], has bool [R, F, S])``."""
    rg = env["rg"]
    search = _search(env, scene)
    sel = list(range(scene.n_radars)) if sel is None else list(sel)
    nf, n = len(fs[0]), scene.shape[0] * len(xs)
    values = np.full((len(sel), nf, n), np.float32(FILL))
    for k, r in enumerate(sel):
        if len(scene.vols[r].gate_x) == 0:
            continue
        got = rg.mosaic_section_fields_device(search, xs, ys, *_call(env, fs, shared, [r]), weighting=weighting,
                                              fill_value=FILL, radars=[r])
        values[k] = got.cpu().numpy().reshape(nf, n)
    return values, values != np.float32(FILL)


def _section_d(scene, xs, ys, sel=None):
    sel = range(scene.n_radars) if sel is None else sel
    return np.stack([cs.section_d(scene, r, xs, ys).ravel() for r in sel])


@pytest.mark.parametrize("nf", [1, 3])
@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("name", ["scene16", "tie"])
def test_section_combine_is_the_fold_of_the_per_radar_sections(env, name, weighting, nf):
    rg = env["rg"]
    scene = cs.scene(name)
    search = _search(env, scene)
    xs, ys = cs.path(name)
    assert len(xs) % 4 == 3
    d = _section_d(scene, xs, ys)
    fs, shared = cs.field_set(scene, nf)
    values, has = _per_radar(env, scene, xs, ys, fs, shared, weighting)
    assert has.any(axis=0).sum() > 30 * nf and (~has.any(axis=0)).sum() > 20 * nf and (has.sum(axis=0) >= 2).sum() > 20 * nf
    everyone = list(range(scene.n_radars))
    for combine in cs.COMBINES:
        label = f"{name} {weighting} {nf} field(s) {combine}"
        want, who = _expect(values, has, d, combine)
        got, radar = rg.mosaic_section_fields_device(search, xs, ys, *_call(env, fs, shared, everyone), weighting=weighting,
                                                     fill_value=FILL, combine=combine, return_radar=True)
        assert tuple(got.shape) == (nf, scene.shape[0], len(xs)) == tuple(radar.shape)
        _same_bits(got, want, label)
        _same_radar(radar, who, label)
        alone = rg.mosaic_section_fields_device(search, xs, ys, *_call(env, fs, shared, everyone), weighting=weighting,
                                                fill_value=FILL, combine=combine)
        _same_bits(alone, want, label + " (no radar map)")
    if name == "tie":                          # on the mirror column the two mirror radars tie in D; the earlier one is named
        p, q = cs.TIE_MIRROR
        on = np.tile(xs == 0.0, scene.shape[0])
        _, wnear = _expect(values, has, d, "nearest_radar")
        tied = on & has[p, 0] & has[q, 0] & (d[p] == d[q])
        assert tied.sum() >= 3 and not (wnear[0][tied] == q).any() and (wnear[0][tied] == p).any()
        assert (values[p, 0][tied] != values[q, 0][tied]).all()


@pytest.mark.parametrize("name", ["scene16", "tie"])
def test_section_mean_through_the_new_entry_point_is_the_old_entry_point(env, name):
    rg, torch, native = env["rg"], env["torch"], env["native"]
    from radar_processor_amd.mosaic import _concat_on_device, _offsets
    from radar_processor_amd.roi_grid import pack_and_grid
    lib = native.load_library()
    scene = cs.scene(name)
    search = _search(env, scene)
    xs, ys = cs.path(name)
    nz, n = scene.shape[0], len(xs)
    sel = list(range(scene.n_radars))
    counts = [search.n_gates[r] for r in sel]
    all_points = rg.mosaic_section_points(search, xs, ys)
    points = [None if np.isnan(all_points[r][0]).all() else
              (torch.from_numpy(all_points[r][0]).to(env["dev"]), torch.from_numpy(all_points[r][1]).to(env["dev"])) for r in sel]
    table = search.section_table(sel, _offsets(counts)[:-1], points)
    n_total = sum(counts)
    for weighting in WEIGHTINGS:
        for nf in (1, 3):
            fs, shared = cs.field_set(scene, nf)
            fields, masks, shared_t = _call(env, fs, shared, sel)
            cat = _concat_on_device(fields, masks, shared_t, counts, nf, torch, env["dev"])
            outs = []
            for which in ("old", "new"):
                def launch(packed, nf_, stride, out_view, stream):
                    head = (table, len(sel), nz, n, search.min_radius, search.beam_factor, native.WEIGHTINGS[weighting],
                            native.ptr(packed), nf_, stride, n_total, float("nan"), native.ptr(out_view))
                    if which == "old":
                        rc = lib.rg_roi_section_mosaic_f32(*head, stream)
                    else:
                        rc = lib.rg_roi_section_mosaic_combine_f32(*head, native.COMBINES["mean"], None, stream)
                    native.check(rc, which)
                outs.append(pack_and_grid(env["dev"], n_total, *cat, None, (nz, n), launch).cpu().numpy())
            assert np.isfinite(outs[0]).sum() > 30 * nf
            np.testing.assert_array_equal(outs[0].view(np.int32), outs[1].view(np.int32), err_msg=f"{weighting} {nf}")
            via_python = rg.mosaic_section_fields_device(search, xs, ys, fields, masks, shared_t, weighting=weighting)
            np.testing.assert_array_equal(via_python.cpu().numpy().view(np.int32), outs[0].view(np.int32))


@pytest.mark.parametrize("combine", cs.COMBINES)
def test_section_one_radar_and_the_colocated_pair(env, combine):
    rg = env["rg"]
    scene = cs.tie_scene()
    search = _search(env, scene)
    xs, ys = cs.path("tie")
    a, b = cs.TIE_TWINS
    for nf in (1, 3):
        fs, shared = cs.field_set(scene, nf)
        # one radar alone under the rule is its mean; the map holds its index or 255
        r = cs.TIE_MIRROR[1]
        call = _call(env, fs, shared, [r])
        mean = rg.mosaic_section_fields_device(search, xs, ys, *call, weighting="cressman", radars=[r])
        got, radar = rg.mosaic_section_fields_device(search, xs, ys, *call, weighting="cressman", radars=[r], combine=combine,
                                                     return_radar=True)
        _same_bits(got, mean.cpu().numpy(), f"radar {r}")
        _, has = _per_radar(env, scene, xs, ys, fs, shared, "cressman", sel=[r])
        _same_radar(radar, np.where(has[0], np.uint8(r), np.uint8(255)), f"radar {r}")
        assert has.any() and not has.all()
        # the twins in both table orders: the earlier position wins, the values do not change
        outs = []
        for sel in ([a, b], [b, a]):
            got, radar = rg.mosaic_section_fields_device(search, xs, ys, *_call(env, fs, shared, sel), weighting="barnes2",
                                                         fill_value=FILL, radars=sel, combine=combine, return_radar=True)
            outs.append((got.cpu().numpy(), radar.cpu().numpy()))
        np.testing.assert_array_equal(outs[0][0].view(np.int32), outs[1][0].view(np.int32))
        filled = outs[0][0] != np.float32(FILL)
        assert filled.sum() > 10 * nf and (outs[0][1][filled] == a).all() and (outs[1][1][filled] == b).all()
        assert (outs[0][1][~filled] == 255).all() and (outs[1][1][~filled] == 255).all()


def test_section_subset_maps_positions_back_to_search_indices(env):
    rg = env["rg"]
    scene = cs.scene("scene16")
    search = _search(env, scene)
    xs, ys = cs.path("scene16")
    sel = [13, 2, 9, 7, 4, 15, 0, 6, 5]
    for nf in (1, 3):
        fs, shared = cs.field_set(scene, nf)
        values, has = _per_radar(env, scene, xs, ys, fs, shared, "nearest", sel=sel)
        d = _section_d(scene, xs, ys, sel)
        for combine in cs.COMBINES:
            want, who = _expect(values, has, d, combine)
            got, radar = rg.mosaic_section_fields_device(search, xs, ys, *_call(env, fs, shared, sel), weighting="nearest",
                                                         fill_value=FILL, radars=sel, combine=combine, return_radar=True)
            _same_bits(got, want, combine)
            lut = np.full(256, 255, dtype=np.uint8)
            lut[:len(sel)] = sel
            _same_radar(radar, lut[who], combine)
            seen = set(np.unique(radar.cpu().numpy()).tolist())
            assert seen <= set(sel) | {255} and len(seen - {255}) >= 3 and 7 not in seen and 0 not in seen


@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("name", ["scene16", "tie"])
def test_section_values_lie_within_the_bound_of_the_named_radars_float64_mean(env, name, weighting):
    """As in tests/test_gpu_mosaic_combine.py, with the brute-force neighbours of every radar at the points in its frame
    (mosaic_section_scenes.radar_pairs): the fill exactly where no radar has a live neighbour, every filled sample within
    oracle.mean_error_bound (DELTA_K2) of the float64 mean of the radar the map names, and under nearest_radar that radar the
    argmin of the float64 D among the radars with a live neighbour, the earliest of equals."""
    rg = env["rg"]
    scene = cs.scene(name)
    search = _search(env, scene)
    xs, ys = cs.path(name)
    for nf in (1, 3):
        fs, shared = cs.field_set(scene, nf)
        d = _section_d(scene, xs, ys)
        stats = [[cs.radar_stats(scene, weighting, fs, shared, k, r, cs.section_pairs(scene, weighting, r, xs, ys, "combine"))
                  for r in range(scene.n_radars)] for k in range(nf)]
        for combine in cs.COMBINES:
            got, radar = rg.mosaic_section_fields_device(search, xs, ys, *_call(env, fs, shared, range(scene.n_radars)),
                                                         weighting=weighting, fill_value=FILL, combine=combine,
                                                         return_radar=True)
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
                    ratio = oracle.bound_ratio(got[k][at][fin], {key: v[fin] for key, v in sub.items()},
                                               oracle.DELTA_K2[weighting])
                    assert ratio.max(initial=0.0) <= 1.0, (combine, k, r, float(ratio.max()))
                    odd = got[k][at][~fin]
                    assert np.all(np.isnan(odd) | (odd == sub["m"][~fin].astype(np.float32))) and not np.isfinite(odd).any()
                    checked += int(fin.sum())
                assert checked > 30, checked


def test_the_numpy_convenience_takes_the_rule(env):
    rg, torch = env["rg"], env["torch"]
    from radar_processor_amd.gridding import _coerce_filters, _host_field
    import mosaic_section_scenes as mss
    scene = cs.scene("scene16")
    fields = [np.ma.array(np.ma.getdata(v.fields["DBZH"]), mask=np.ma.getmaskarray(v.fields["DBZH"])) for v in scene.vols]
    kw = dict(min_radius=scene.min_radius, beam_factor=scene.beam_factor, toa=scene.toa)
    xs, ys, s = rg.section_path(mss.VERTICES, 1385.0)
    search = rg.MosaicSearch.for_path(scene.radars(), xs, ys, scene.limits[0], scene.shape[0], **kw)
    host = [_host_field(f, _coerce_filters(None)) for f in fields]
    f_t = [[torch.from_numpy(v).to(env["dev"])] for v, _ in host]
    m_t = [[torch.from_numpy(m).to(env["dev"])] for _, m in host]
    for combine in ("mean",) + cs.COMBINES:
        got, dist = rg.mosaic_vertical_section(scene.radars(), fields, mss.VERTICES, 1385.0, scene.limits[0], scene.shape[0],
                                               combine=combine, **kw)
        want = rg.mosaic_section_fields_device(search, xs, ys, f_t, m_t, combine=combine)[0].cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (scene.shape[0], len(xs)) and np.isfinite(got).sum() > 50
        np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))
        np.testing.assert_array_equal(dist, s)
