"""The three routes from a ``PlaneProducts`` request to its planes agree, bit for bit, with each other and with the public
single-product functions on the same grids:

* ``VolumeBatch(RoiSearch).grid_shard(products=spec)`` against ``ProductPlan(spec, search).planes_of_grids`` on the grids
  ``roi_grid_fields_device`` returns for the same field-volumes;
* ``mosaic_fields_device(MosaicSearch, products=spec)`` (one radar at the origin) against the same on its own grids;
* ``grid_products_device(geometry, products=spec, fused=False)`` against ``column_argmax`` / ``column_min`` / ``column_mean`` /
  ``constant_altitude_ppi`` / ``constant_elevation_ppi`` / ``column_profile`` on ``grid_fields_device``'s grids.

One synthetic radar of 4800 gates on grids of 15 and 24 columns (the column kernels' one-column and 16-byte paths), five
levels with the window strictly inside, a CAPPI below the grid, one on a level and one blended between two interior levels.
Planes are compared through integer views, so NaNs count; there is no tolerance."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = ((5, 3, 5), (5, 4, 6))
LIMITS = ((1000.0, 5000.0), (-40e3, 40e3), (-40e3, 40e3))
MIN_RADIUS = 4000.0                      # coarse lattice: most voxels have neighbours, some have none
WINDOW = dict(z_min_idx=1, z_max_idx=3)
REQUEST = dict(colmax=True, argmax=True, colmin=True, colmean=True, cappi=(500.0, 3000.0, 3500.0), ppi=(0.5, 1.5),
               ppi_interpolation="linear", echo_top=(10.0, 20.0), echo_base=(10.0,), vil=True, **WINDOW)
NAMES = ("DBZH", "ZDR")


@pytest.fixture(scope="module")
def env():
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd.plane_products import RECORD_KEYS, ProductPlan
    rg.load_library()
    return dict(torch=torch, rg=rg, dev=torch.device("cuda", 0), keys=list(RECORD_KEYS), ProductPlan=ProductPlan,
                spec=rg.PlaneProducts(**REQUEST))


@functools.lru_cache(maxsize=None)
def volumes():
    """Two volumes of one radar (same gates); DBZH goes with its mask, ZDR without one."""
    from radar_processor_amd import synthetic
    vols = [synthetic.make_volume(n_elev=10, n_az=30, n_gates=16, seed=seed, fields=NAMES, max_range_m=64e3)
            for seed in (20, 14)]
    host = [{"DBZH": (np.ma.getdata(v.fields["DBZH"]), np.ma.getmaskarray(v.fields["DBZH"]).astype(np.uint8)),
             "ZDR": (np.ma.getdata(v.fields["ZDR"]), None)} for v in vols]
    return vols[0], host


def device_fields(env, host_volumes):
    torch, dev = env["torch"], env["dev"]
    pairs = [vol[name] for vol in host_volumes for name in NAMES]
    return ([torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for v, _ in pairs],
            [None if m is None else torch.from_numpy(m).to(dev) for _, m in pairs])


def bits(torch, plane):
    return plane.contiguous().view(torch.int64 if plane.dtype == torch.float64 else torch.int32)


def assert_same_records(env, got, want, label):
    """Same keys in the canonical order, same sub-keys in the same order, same dtypes, same bits."""
    torch = env["torch"]
    assert len(got) == len(want), label
    for k, (a, b) in enumerate(zip(got, want)):
        assert list(a) == env["keys"] and list(b) == env["keys"], (label, k, list(a), list(b))
        for key in env["keys"]:
            if isinstance(b[key], dict):
                assert list(a[key]) == list(b[key]), (label, k, key)
                planes = [(a[key][s], b[key][s], (key, s)) for s in b[key]]
            else:
                planes = [(a[key], b[key], key)]
            for p, q, what in planes:
                assert p.dtype == q.dtype and p.shape == q.shape, (label, k, what)
                assert torch.equal(bits(torch, p), bits(torch, q)), (label, k, what)


def public_records(env, grids, spec_like):
    """The request through the public single-product functions, one grid at a time."""
    rg = env["rg"]
    recs = []
    for g in grids:
        colmax, argmax = rg.column_argmax(g, **WINDOW)
        rec = dict(colmax=colmax, argmax=argmax, colmin=rg.column_min(g, **WINDOW), colmean=rg.column_mean(g, **WINDOW),
                   cappi={a: rg.constant_altitude_ppi(g, spec_like, a, "linear") for a in REQUEST["cappi"]},
                   ppi={e: rg.constant_elevation_ppi(g, spec_like, e, "linear") for e in REQUEST["ppi"]})
        rec.update(rg.column_profile(g, spec_like, echo_top=REQUEST["echo_top"], echo_base=REQUEST["echo_base"], vil=True,
                                     **WINDOW))
        recs.append(rec)
    return recs


def assert_not_vacuous(env, rec):
    """The DBZH record of the first volume: echoes above 10 dBZ, a VIL, and the all-NaN plane below the grid."""
    torch = env["torch"]
    assert torch.isfinite(rec["colmax"]).any() and torch.isfinite(rec["echo_top"][10.0]).any()
    assert torch.isfinite(rec["vil"]).any() and torch.isfinite(rec["cappi"][3500.0]).any()
    assert torch.isnan(rec["cappi"][500.0]).all()
    assert rec["ppi"][1.5].dtype == torch.float64 and rec["argmax"].dtype == torch.int32


@pytest.mark.parametrize("shape", SHAPES)
def test_batch_on_a_roi_search_is_the_plan_on_its_grids(env, shape, caplog):
    rg, dev = env["rg"], env["dev"]
    from radar_processor_amd import batch
    vol, host = volumes()
    search = rg.RoiSearch(vol.gate_x, vol.gate_y, vol.gate_z, shape, LIMITS, min_radius=MIN_RADIUS, device=dev)
    vb = batch.VolumeBatch(search, list(NAMES), device=dev)
    assert vb.volumes_per_pass >= 2                                   # both volumes share one pass, as gridded below
    with caplog.at_level("WARNING", logger="radar_grid.products"):
        got = vb.grid_shard(host, products=env["spec"])
    warned = [r.getMessage() for r in caplog.records if r.name == "radar_grid.products"]
    assert warned == ["Altitude 500.0m is outside grid range [1000.0, 5000.0]m"]           # once per call, not per field
    fields, masks = device_fields(env, host)
    grids = rg.roi_grid_fields_device(search, fields, masks)
    want = env["ProductPlan"](env["spec"], search).planes_of_grids(grids)
    assert sorted(got) == [0, 1]
    assert_same_records(env, got[0] + got[1], want, ("batch", shape))
    assert_same_records(env, want, public_records(env, grids, search), ("batch, public", shape))
    assert_not_vacuous(env, got[0][0])


@pytest.mark.parametrize("shape", SHAPES)
def test_mosaic_search_is_the_plan_on_its_grids(env, shape):
    rg, dev = env["rg"], env["dev"]
    vol, host = volumes()
    ms = rg.MosaicSearch([(vol.gate_x, vol.gate_y, vol.gate_z, (0.0, 0.0, 0.0))], shape, LIMITS, min_radius=MIN_RADIUS,
                         device=dev)
    fields, masks = device_fields(env, host[:1])
    got = rg.mosaic_fields_device(ms, [fields], [masks], products=env["spec"])
    grids = rg.mosaic_fields_device(ms, [fields], [masks])
    want = env["ProductPlan"](env["spec"], ms).planes_of_grids(grids)
    assert_same_records(env, got, want, ("mosaic", shape))
    assert_same_records(env, want, public_records(env, grids, ms), ("mosaic, public", shape))
    assert_not_vacuous(env, got[0])


@pytest.mark.parametrize("shape", SHAPES)
def test_csr_geometry_unfused_is_the_public_functions_on_its_grids(env, shape, tmp_path):
    rg = env["rg"]
    vol, host = volumes()
    geom = rg.compute_grid_geometry(vol.gate_x, vol.gate_y, vol.gate_z, shape, LIMITS, str(tmp_path), min_radius=MIN_RADIUS)
    fields, masks = device_fields(env, host[:1])
    got = rg.grid_products_device(geom, fields, masks, products=env["spec"], fused=False)
    grids = rg.grid_fields_device(geom, fields, masks)
    assert_same_records(env, got, public_records(env, grids, geom), ("csr", shape))
    assert_same_records(env, got, env["ProductPlan"](env["spec"], geom).planes_of_grids(grids), ("csr, plan", shape))
    assert_not_vacuous(env, got[0])
