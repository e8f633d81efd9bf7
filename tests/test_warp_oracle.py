"""CPU-side checks of the Web Mercator warp (no GPU needed): the NumPy float64 restatement of the pixel map
(tests/warp_oracle.py) against a 40-digit evaluation, the cap on pixels that rounding may decide either way, the host
helpers of ``radar_processor_amd/warp.py`` (rasters, tiles, the Mercator maps), every refusal of the Python surface before
any device work, and the ABI bookkeeping."""
import json
import math
import os
import re

import numpy as np
import pytest

import radar_processor_amd as rg
import warp_oracle as wo
from conftest import REPO
from radar_processor_amd import _native, warp

BOUNDS = os.path.join(REPO, "profiles", "warp_bounds.json")
ORACLE_BOUND_M = 1e-8          # the floor profiles/georef_bounds.json records for the georef restatement


# ---- the restatement -------------------------------------------------------------------------------------------------------
def test_scenes_are_what_the_module_says():
    for name in wo.MAIN:
        r = wo.scene(name).raster
        assert 34 <= r.height <= 39 and 47 <= r.width <= 58, (name, r)
        fx, fy, c = wo.mapped(name)
        inside = wo.nearest_index(fx, fy, c, wo.scene(name).lattice)[0].mean()
        assert 88 <= round(100 * inside) <= 98, (name, inside)
        for f in wo.FACTORS[1:]:                             # from factor 4 on every level of every scene has clipped blocks
            assert r.height % f and r.width % f
        assert max(r.height, r.width) < 64                   # ... and 64 exceeds both axes
    sizes = [wo.scene(n).raster for n in wo.MAIN]            # factor 2 meets an odd height (39) and an odd width (47)
    assert any(r.height % 2 for r in sizes) and any(r.width % 2 for r in sizes)
    assert wo.scene("antimeridian").raster.x_min < -math.pi * wo.A_MERCATOR       # the raster runs past -pi a
    assert [(wo.scene(n).raster.height, wo.scene(n).raster.width) for n in ("one_pixel", "one_row", "one_column")] == \
        [(1, 1), (1, 54), (38, 1)]
    fine = wo.scene("rma1_fine").raster
    assert fine.width > 2 * 64 and fine.height > 3 * 32                          # several kernel tiles both ways
    # the tile cuts the grid's edge: part of it inside, most of it not
    fx, fy, c = wo.mapped("tile_edge")
    assert 0.05 < wo.nearest_index(fx, fy, c, wo.scene("tile_edge").lattice)[0].mean() < 0.5
    assert wo.scene("tile_edge").raster == tuple(rg.mercator_tile(6, 20, 38, 64))
    # the contract scene: every pixel of the world tile lands INSIDE the plane, more than half of them beyond the limit
    far = wo.scene("far_hemisphere")
    fx, fy, c = wo.mapped("far_hemisphere")
    in_plane = (fx + 0.5 >= 0) & (fx + 0.5 < far.lattice.nx) & (fy + 0.5 >= 0) & (fy + 0.5 < far.lattice.ny)
    assert in_plane.all() and 0.5 < (c >= wo.LIMIT).mean() < 0.6
    assert far.raster == tuple(rg.mercator_tile(0, 0, 0))
    # sources name their pixel; the RGBA of a source pixel is never the fill
    assert wo.index_plane((37, 53))[36, 52] == 36052.0 and wo.index_rgba((37, 53))[36, 52].tolist() == [36, 52, 0, 255]
    # the single finite pixel survives the 0.5 rule somewhere
    fx, fy, c = wo.mapped("rma1_fine")
    kept = ~wo.sample_bilinear(wo.bilinear_source("rma1_fine", "one_finite"), fx, fy, c, wo.scene("rma1_fine").lattice, np.nan)[2]
    assert 0 < kept.sum() < 20


def test_restatement_against_40_digits_on_every_pixel():
    """|NumPy float64 - mpmath| < 1e-8 m on both plane coordinates of every pixel of the three main scenes; the measured
    maximum is what profiles/warp_bounds.json records (held to a factor of two: the last bits of the host's libm)."""
    now = wo.oracle_summary()
    print("oracle vs mpmath, metres:", json.dumps(now))
    for name, err in now["per_scene_m"].items():
        assert err < ORACLE_BOUND_M, (name, err)
    with open(BOUNDS) as f:
        rec = json.load(f)["oracle_vs_mpmath"]
    assert sorted(rec["per_scene_m"]) == sorted(wo.MAIN) and rec["pixels"] == now["pixels"]
    assert rec["max_m"] == max(rec["per_scene_m"].values()) < ORACLE_BOUND_M
    assert 0.5 * now["max_m"] <= rec["max_m"] <= 2.0 * now["max_m"]


def test_recorded_kernel_numbers_are_within_the_bound():
    """profiles/warp_bounds.json, the part measured on the GPU (tests/test_gpu_warp.py asserts the same live)."""
    with open(BOUNDS) as f:
        rec = json.load(f)["bilinear_vs_oracle"]
    assert sorted(rec) == sorted(wo.SCENES)
    for name, kinds in rec.items():
        assert sorted(kinds) == sorted(wo.BILINEAR_SOURCES)
        for kind, r in kinds.items():
            assert r["fill_set_differs"] == 0 and r["pixels"] == wo.scene(name).pixels, (name, kind)
            assert r["worst_excess"] is None or r["worst_excess"] <= 0.0, (name, kind)


@pytest.mark.parametrize("name", wo.SCENES)
def test_undecided_pixels_stay_under_the_cap(name):
    cap = wo.UNDECIDED_CAP * wo.scene(name).pixels
    assert wo.undecided_nearest(name).sum() <= cap
    for kind in wo.BILINEAR_SOURCES:
        assert wo.undecided_bilinear(name, wo.bilinear_source(name, kind)).sum() <= cap, kind


def test_known_answers_of_the_pixel_map():
    # a raster centred on the origin: the central pixel pair straddles (0, 0); north is up and east is right
    for origin in (wo.RMA1, (10.0, 70.0), (-179.5, 5.0)):
        x0, y0 = (float(v) for v in rg.lonlat_to_mercator(*origin))
        r = wo.Raster(x0 - 2 * 1000.0, y0 + 2 * 1000.0, 1000.0, 4, 4)
        Xg, Yg, c = wo.pixel_map(r, origin)
        assert (np.diff(Xg, axis=1) > 0).all() and (np.diff(Yg, axis=0) < 0).all()
        assert abs(Xg[1, 1] + Xg[1, 2]) < 1e-6 and abs(Yg[1, 1] + Yg[2, 1]) < 1.0 and c.max() < 1e-3     # the origin in the middle
        # a Mercator pixel of 1 km is cos(lat) km on the ground (times the two spheres' ratio)
        want = 1000.0 * math.cos(math.radians(origin[1])) * wo.R_EARTH / wo.A_MERCATOR
        assert abs((Xg[1, 2] - Xg[1, 1]) / want - 1.0) < 1e-4
    # the map is periodic in X
    s = wo.scene("antimeridian")
    shifted = s.raster._replace(x_min=s.raster.x_min + 2.0 * math.pi * wo.A_MERCATOR)
    a, b = wo.pixel_map(s.raster, s.origin), wo.pixel_map(shifted, s.origin)
    assert max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max()) < 1e-6


def test_restated_sampling_and_overview_rules_on_hand_made_cases():
    lat = wo.lattice((3, 4), ((0.0, 2.0), (0.0, 3.0)))
    src = wo.index_plane((3, 4))
    fx, fy = np.array([[0.49, 0.51, 3.49, 3.51, -0.51]]), np.array([[1.49, 1.51, 2.49, 2.51, 0.0]])
    c = np.zeros_like(fx)
    got = wo.sample_nearest(src[None], fx, fy, c, lat, -1.0)[0]
    assert got.tolist() == [[1000.0, 2001.0, 2003.0, -1.0, -1.0]]
    assert wo.sample_nearest(src[None], fx, fy, c + wo.LIMIT, lat, -1.0)[0].tolist() == [[-1.0] * 5]
    # bilinear: the middle of a cell is the mean of its taps; a NaN tap is skipped; below half the weight it is fill
    out, wsum, filled = wo.sample_bilinear(src, np.array([[0.5]]), np.array([[0.5]]), np.zeros((1, 1)), lat, np.nan)
    assert out[0, 0] == (0 + 1 + 1000 + 1001) / 4 and wsum[0, 0] == 1.0
    holed = src.copy()
    holed[0, 0] = np.nan
    out, wsum, filled = wo.sample_bilinear(holed, np.array([[0.5, 0.2]]), np.array([[0.5, 0.2]]), np.zeros((1, 2)), lat, np.nan)
    assert out[0, 0] == (1 + 1000 + 1001) / 3 and wsum[0, 0] == 0.75 and filled.tolist() == [[False, True]]
    assert wo.adjacent_difference(src) == 1001.0
    # overviews
    img = np.arange(35, dtype=np.float32).reshape(5, 7)
    assert wo.overview_nearest(img, 2).tolist() == [[8, 10, 12, 13], [22, 24, 26, 27], [29, 31, 33, 34]]
    assert wo.overview_nearest(img, 64).tolist() == [[34.0]]
    avg = wo.overview_average(img, 4)
    assert avg.shape == (2, 2) and avg[0, 0] == np.mean([0, 1, 2, 3, 7, 8, 9, 10, 14, 15, 16, 17, 21, 22, 23, 24])
    assert avg[1, 1] == np.mean([32, 33, 34])
    img[4, 4:] = [np.nan, np.inf, -np.inf]
    assert np.isnan(wo.overview_average(img, 4)[1, 1])


# ---- the host helpers ------------------------------------------------------------------------------------------------------
def test_mercator_maps_round_trip_and_known_values():
    x, y = rg.lonlat_to_mercator([0.0, 180.0, -64.19], [0.0, 0.0, -31.44])
    assert x[0] == 0.0 and y[0] == 0.0 and abs(x[1] - math.pi * 6378137.0) < 1e-8
    assert abs(y[2] - 6378137.0 * math.log(math.tan(math.pi / 4 + math.radians(-31.44) / 2))) < 1e-6
    lat_edge = float(rg.mercator_to_lonlat(0.0, math.pi * 6378137.0)[1])
    assert abs(lat_edge - 85.0511287798066) < 1e-10                        # the square world's edge
    lon, lat = np.meshgrid(np.linspace(-179.0, 179.0, 41), np.linspace(-85.0, 85.0, 37))
    blon, blat = rg.mercator_to_lonlat(*rg.lonlat_to_mercator(lon, lat))
    assert np.abs(blon - lon).max() < 1e-12 and np.abs(blat - lat).max() < 1e-12
    assert warp.MERCATOR_RADIUS == wo.A_MERCATOR


def test_raster_properties():
    r = rg.MercatorRaster(100.0, 900.0, 2.5, 40, 20)
    assert r.bounds == (100.0, 850.0, 200.0, 900.0) and r.transform == (100.0, 2.5, 0.0, 900.0, 0.0, -2.5)
    assert tuple(r) == (100.0, 900.0, 2.5, 40, 20)
    assert [name for name, _ in _native.MercatorRaster._fields_] == list(r._fields)


@pytest.mark.parametrize("name", wo.MAIN)
def test_mercator_raster_for_contains_every_node(name):
    shape, limits, origin = wo.GRIDS[name]
    r = rg.mercator_raster_for((5,) + shape, ((0.0, 1e4),) + limits, origin + (250.0,))      # the gridders' 3-D arguments ...
    assert r == rg.mercator_raster_for(shape, limits, origin) == wo.scene(name).raster        # ... or the plane's own
    lat = wo.lattice(shape, limits)
    assert r.pixel == min(lat.step_x, lat.step_y) / math.cos(math.radians(origin[1]))
    yc, xc = (lat.y_lo + np.arange(lat.ny) * lat.step_y)[:, None], (lat.x_lo + np.arange(lat.nx) * lat.step_x)[None, :]
    lon, lat_deg = rg.grid_to_geographic(xc, yc, *origin)
    lon = origin[0] + ((lon - origin[0] + 180.0) % 360.0 - 180.0)
    mx, my = rg.lonlat_to_mercator(lon, lat_deg)
    west, south, east, north = r.bounds
    assert west < mx.min() and mx.max() < east and south < my.min() and my.max() < north
    # ... with no more slack than the half cell around the outer nodes and the last, partly used pixel
    assert mx.min() - west < 1.2 * r.pixel and north - my.max() < 1.2 * r.pixel
    assert east - mx.max() < 2.2 * r.pixel and my.min() - south < 2.2 * r.pixel
    if name == "antimeridian":
        assert west < -math.pi * 6378137.0 < east                                             # one connected raster
    # every node is the nearest sample of the pixel it falls in, or of a neighbour: the map and the raster agree
    fx, fy, _ = wo.mapped(name)
    col, row = ((mx - r.x_min) / r.pixel).astype(int), ((r.y_max - my) / r.pixel).astype(int)
    assert np.abs(fx[row, col] - np.arange(lat.nx)[None, :]).max() < 1.0 and np.abs(fy[row, col] - np.arange(lat.ny)[:, None]).max() < 1.0
    half = rg.mercator_raster_for(shape, limits, origin, pixel_size=r.pixel / 2.0)
    assert half.pixel == r.pixel / 2.0 and (half.x_min, half.y_max) == (r.x_min, r.y_max) and 2 * r.width - 1 <= half.width <= 2 * r.width


def test_tiles():
    world = rg.mercator_tile(0, 0, 0)
    half = math.pi * 6378137.0
    assert world == (-half, half, 2.0 * half / 256, 256, 256) and world.bounds == (-half, -half, half, half)
    for z, x, y in ((0, 0, 0), (3, 5, 2), (6, 20, 38), (17, 44201, 77003), (29, 2 ** 29 - 1, 0)):
        parent = rg.mercator_tile(z, x, y, size=64)
        kids = [[rg.mercator_tile(z + 1, 2 * x + i, 2 * y + j, size=64) for i in (0, 1)] for j in (0, 1)]
        for row in kids:
            for k in row:
                assert k.pixel == parent.pixel / 2.0 and (k.width, k.height) == (64, 64)
        # the children's outer corners are the parent's, their inner edges one line each way: an exact partition
        assert (kids[0][0].x_min, kids[0][0].y_max) == (parent.x_min, parent.y_max)
        assert kids[1][0].x_min == parent.x_min and kids[0][1].y_max == parent.y_max
        assert kids[0][1].x_min == kids[1][1].x_min and kids[1][0].y_max == kids[1][1].y_max
        # ... which is the parent's middle line, and the next tile's edge the parent's far one, to an ulp at 2e7 m (each edge
        # is rounded once from 2 pi a (i / 2^z - 1/2); x_min + width * pixel rounds again)
        assert abs(kids[0][1].x_min - (parent.x_min + 32 * parent.pixel)) <= 4e-9
        assert abs(kids[1][0].y_max - (parent.y_max - 32 * parent.pixel)) <= 4e-9
        assert abs(kids[1][1].bounds[2] - parent.bounds[2]) <= 4e-9 and abs(kids[1][1].bounds[1] - parent.bounds[1]) <= 4e-9
        if x + 1 < 2 ** z:
            assert abs(rg.mercator_tile(z, x + 1, y, size=64).x_min - parent.bounds[2]) <= 4e-9
    for bad in ((-1, 0, 0), (31, 0, 0), (2, 4, 0), (2, 0, 4), (2, -1, 0), (1.5, 0, 0)):
        with pytest.raises(ValueError):
            rg.mercator_tile(*bad)
    with pytest.raises(ValueError):
        rg.mercator_tile(1, 0, 0, size=0)


# ---- refusals: all before any device call ----------------------------------------------------------------------------------
def test_every_refusal_raises_without_a_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_native, "load_library", no_device)
    monkeypatch.setattr(_native, "canonical_device", no_device)
    monkeypatch.setattr(_native, "device", no_device)
    s = wo.scene("rma1")
    plane, rgba = wo.index_plane(s.shape), wo.index_rgba(s.shape)
    ok = dict(grid_limits=s.limits, grid_origin=s.origin, raster=s.raster)

    def warp_refuses(match, data=plane, **kw):
        with pytest.raises(ValueError, match=match):
            rg.warp_to_mercator_device(data, **{**ok, **kw})

    for bad in ((10.0, 90.5), (np.nan, 45.0), (10.0,)):
        warp_refuses(None, grid_origin=bad)
        with pytest.raises(ValueError):
            rg.mercator_raster_for(s.shape, s.limits, bad)
        with pytest.raises(ValueError):
            rg.web_mercator_rgba(plane, s.limits, bad, np.zeros((7, 4), np.uint8), 0.0, 1.0)
    for bad_r in (0.0, -1.0, np.nan, np.inf):
        warp_refuses("R must be finite and positive", R=bad_r)
        with pytest.raises(ValueError, match="R must be finite and positive"):
            rg.mercator_raster_for(s.shape, s.limits, s.origin, R=bad_r)
    for bad in (s.raster._replace(pixel=0.0), s.raster._replace(pixel=-1.0), s.raster._replace(pixel=np.nan),
                s.raster._replace(x_min=np.inf), s.raster._replace(y_max=np.nan), s.raster._replace(width=-1),
                s.raster._replace(height=2 ** 31), s.raster._replace(width=3.5), (1.0, 2.0, 3.0), None):
        warp_refuses("raster", raster=bad)
    warp_refuses("method must be one of", method="cubic")
    warp_refuses("nearest' only", data=rgba, method="bilinear")
    warp_refuses("data must be float32", data=plane.astype(np.float64))
    warp_refuses("data must be float32", data=rgba[:, :, :3])
    warp_refuses("data must be float32", data=plane.ravel())
    warp_refuses("data must be float32", data=plane[None, None])
    warp_refuses("at least 2 x 2", data=plane[:1])
    warp_refuses("at least 2 x 2", data=plane[:, :1])
    warp_refuses("finite and increasing", grid_limits=((1.0, 1.0), (0.0, 2.0)))
    warp_refuses("finite and increasing", grid_limits=((0.0, 1.0), (0.0, np.inf)))
    warp_refuses("bad grid shape", grid_limits=((0.0, 1.0),))
    warp_refuses("out must be a tensor of shape", out=np.zeros((s.raster.height, s.raster.width), np.float32))
    with pytest.raises(ValueError, match="pixel_size"):
        rg.mercator_raster_for(s.shape, s.limits, s.origin, pixel_size=0.0)
    with pytest.raises(ValueError, match="at least 2 x 2"):
        rg.mercator_raster_for((1, 5), s.limits, s.origin)
    with pytest.raises(ValueError, match="pole"):
        rg.mercator_raster_for(s.shape, s.limits, (0.0, 89.0))

    # the pyramid
    for bad in ((2, 4), 2, "2,4", np.array([2, 4])):
        with pytest.raises(TypeError, match="must be a list or None"):
            rg.overview_pyramid_device(plane, bad)
    with pytest.raises(TypeError, match="must be a string"):
        rg.overview_pyramid_device(plane, [2], resampling=1)
    for name in ("bilinear", "cubic", "mode", "max", "min", "med", "q1", "q3", "rms", "lanczos"):
        with pytest.raises(ValueError, match="average.*nearest") as info:
            rg.overview_pyramid_device(plane, [2], resampling=name)
        assert ("unknown" in str(info.value)) == (name == "lanczos")
    for bad in ([1], [65], [2, 0], [2.5], [True], [-2]):
        with pytest.raises(ValueError, match="2 .. 64"):
            rg.overview_pyramid_device(plane, bad)
    with pytest.raises(ValueError, match="nearest' only"):
        rg.overview_pyramid_device(rgba, [2], resampling="average")
    with pytest.raises(ValueError, match="image must be float32"):
        rg.overview_pyramid_device(plane.astype(np.int32), [2])
    assert rg.overview_pyramid_device(plane, []) == [] and rg.overview_pyramid_device(rgba, [], "Nearest ") == []

    # the chain
    lut = np.zeros((7, 4), np.uint8)
    chain = dict(grid_limits=s.limits, grid_origin=s.origin, lut=lut, vmin=0.0, vmax=1.0)
    for kw, err in ((dict(vmin=2.0), ValueError), (dict(vmax=np.nan), ValueError), (dict(lut=np.zeros((7, 3), np.uint8)), ValueError),
                    (dict(lut=np.zeros((3, 4), np.uint8)), ValueError), (dict(method="cubic"), ValueError),
                    (dict(resampling="mode"), ValueError), (dict(factors=(2,)), TypeError), (dict(factors=[128]), ValueError),
                    (dict(raster=s.raster._replace(pixel=0.0)), ValueError)):
        with pytest.raises(err):
            rg.web_mercator_rgba(plane, **{**chain, **kw})
    for bad_plane in (plane[None], rgba, plane.astype(np.float64)):
        with pytest.raises(ValueError, match="float32"):
            rg.web_mercator_rgba(bad_plane, **chain)


# ---- bookkeeping -----------------------------------------------------------------------------------------------------------
FUNCTIONS = ("rg_warp_mercator_f32", "rg_warp_mercator_rgba8", "rg_overview_f32", "rg_overview_rgba8")


def _struct_members(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [(kind, m.strip()) for kind, decl in re.findall(r"(double|int32_t)\s+([^;]+);", body) for m in decl.split(",")]


def test_abi_bookkeeping_and_exports():
    import ctypes
    header = open(os.path.join(REPO, "include", "radargrid_hip.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t|const char\*)\s+(rg_\w+)\s*\(", header, flags=re.M))
    for name in FUNCTIONS:
        assert name in declared and name in _native.SIGNATURES
    assert "#define RG_VERSION 104" in header and _native.ABI_VERSION == 104
    kinds = {"double": ctypes.c_double, "int32_t": ctypes.c_int32}
    for c_name, mirror, oracle in (("rg_mercator_raster", _native.MercatorRaster, wo.Raster),
                                   ("rg_warp_source", _native.WarpSource, wo.Lattice)):
        members = _struct_members(header, c_name)
        assert [(kinds[k], m) for k, m in members] == [(t, n) for n, t in mirror._fields_]
        assert [m for _, m in members] == list(oracle._fields)
    from radar_processor_amd import build
    assert ("rg_warp.hip", []) in build.SOURCES and build.SOURCES[-1] == ("rg_warp.hip", [])
    lib = rg.load_library(require_device=False)
    assert lib.rg_version() == 104
    for name in FUNCTIONS:
        assert getattr(lib, name).argtypes == _native.SIGNATURES[name][1]
    # the arguments the header declares, by kind, against the ctypes table
    for name in FUNCTIONS:
        args = re.search(r"^int %s\((.*?)\);" % name, header, flags=re.S | re.M).group(1).split(",")
        want = []
        for a in args:
            a = " ".join(a.split())
            want.append(ctypes.POINTER(_native.WarpSource) if "rg_warp_source*" in a else
                        ctypes.POINTER(_native.Georef) if "rg_georef*" in a else
                        ctypes.POINTER(_native.MercatorRaster) if "rg_mercator_raster*" in a else
                        ctypes.c_void_p if ("*" in a or a.startswith("rg_stream_t")) else
                        ctypes.c_float if a.startswith("float ") else ctypes.c_int32)
        assert want == _native.SIGNATURES[name][1], name
    for name in ("MercatorRaster", "lonlat_to_mercator", "mercator_to_lonlat", "mercator_raster_for", "mercator_tile",
                 "warp_to_mercator_device", "overview_pyramid_device", "web_mercator_rgba"):
        assert name in rg.__all__ and getattr(rg, name) is getattr(warp, name)
    assert warp.DEFAULT_OVERVIEW_FACTORS == [2, 4, 8, 16]
    from radar_processor_amd import georef
    assert georef.MAX_ANGULAR_DISTANCE == wo.LIMIT and georef.AEQD_EARTH_RADIUS == wo.R_EARTH
