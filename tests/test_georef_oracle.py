"""CPU-side checks of georeferencing (no GPU needed): the NumPy float64 restatement of the AEQD maps (tests/georef_oracle.py)
against a 40-digit evaluation and known answers, the host maps of ``radar_processor_amd/georef.py`` against the same
evaluation, every refusal of the Python surface and of the two C entry points that is decided before any device work, and the
ABI bookkeeping."""
import json
import math
import os
import re

import numpy as np
import pytest

import georef_oracle as go
import radar_processor_amd as rg
from conftest import REPO
from radar_processor_amd import _native, georef

P = 1 << 12                                  # an aligned address that is never dereferenced
BOUNDS = os.path.join(REPO, "profiles", "georef_bounds.json")
ORACLE_BOUND_M = 1e-7                        # the NumPy restatement against mpmath, every finite scene gate
HOST_BOUND_M = 1e-6                          # geographic_to_grid / grid_to_geographic against mpmath


# ---- the restatement -------------------------------------------------------------------------------------------------------
def test_scenes_are_what_the_module_says():
    assert set(go.SCENES) == {"at_origin", "east_1m", "east_200km", "north_east_1000km", "antimeridian", "lat_80", "equator",
                              "north_mid"}
    assert go.scene("east_200km").x.size == go.LENGTHS[-1] == 4099
    total = 0
    for name in go.SCENES:
        s = go.scene(name)
        assert s.x.dtype == s.y.dtype == np.float32 and s.x.shape == s.y.shape
        assert int((~s.finite).sum()) == go.N_NONFINITE
        r = np.hypot(s.x[s.finite].astype(np.float64), s.y[s.finite].astype(np.float64))
        for want in go.RANGES:                                         # every range of the list is there, the antenna included
            assert (np.abs(r - want) <= 1e-6 * want).sum() >= 180, (name, want)
        for n in go.LENGTHS[1:3]:                                       # the prefixes the kernel tests use hold live gates
            assert s.finite[:n].any()
        total += int(s.finite.sum())
    assert total <= 20000
    assert go.scene("at_origin").radar == go.scene("at_origin").origin
    # the 1 m and the 200 km radars stand where their names say, in the plane of the origin
    for name, east in (("east_1m", 1.0), ("east_200km", 2.0e5)):
        s = go.scene(name)
        x, y = go.forward(*np.radians(s.radar), *s.origin)
        assert abs(x - east) < 1e-8 and abs(y) < 1e-8


def test_restatement_against_40_digits_on_every_finite_gate():
    """|NumPy float64 - mpmath| <= 1e-7 m on both placed coordinates of every finite gate of every scene; the measured
    maximum is what profiles/georef_bounds.json records.  The figure is float64 rounding noise (a few ulp at the earth's
    radius), so it depends on the last bits of the host's sin / cos / atan2: the file is held to a factor of two of it,
    not to equality."""
    now = go.oracle_summary()
    print("oracle vs mpmath, metres:", json.dumps(now))
    assert now["finite_gates"] == sum(int(go.scene(n).finite.sum()) for n in go.SCENES)
    for name, err in now["per_scene_m"].items():
        assert err <= ORACLE_BOUND_M, (name, err)
    with open(BOUNDS) as f:
        rec = json.load(f)["oracle_vs_mpmath"]
    assert sorted(rec["per_scene_m"]) == sorted(go.SCENES) and rec["finite_gates"] == now["finite_gates"]
    assert rec["max_m"] == max(rec["per_scene_m"].values()) <= ORACLE_BOUND_M
    assert 0.5 * now["max_m"] <= rec["max_m"] <= 2.0 * now["max_m"]
    assert rec["per_scene_m"]["at_origin"] == now["per_scene_m"]["at_origin"] == 0.0


def test_recorded_kernel_numbers_are_within_the_bound():
    """profiles/georef_bounds.json, the part measured on the GPU (tests/test_gpu_georef.py asserts the same live)."""
    with open(BOUNDS) as f:
        rec = json.load(f)["kernel_vs_oracle"]
    assert sorted(rec) == sorted(go.SCENES)
    for name, r in rec.items():
        assert r["worst_excess_m"] <= 0.0 and r["nonfinite_as_contract"], name
        assert r["values"] == 2 * int(go.scene(name).finite.sum())
    assert rec["at_origin"]["values_differing"] == 0


def test_known_answers():
    # due north at great-circle distance d -> (0, d), from any centre
    for lon0, lat0 in ((-64.19, -31.44), (179.9, 12.5), (10.0, 0.0), (15.0, 60.0)):
        for d in (1.0, 1234.5, 2.4e5, 1.0e6):
            x, y = go.forward(np.radians(lon0), np.radians(lat0) + d / go.R_EARTH, lon0, lat0)
            assert abs(x) <= 1e-8 and abs(y - d) <= 1e-8 * max(1.0, d / 1e5)
    # the centre maps to the origin and back
    assert go.forward(np.radians(7.0), np.radians(46.0), 7.0, 46.0) == (0.0, 0.0)
    lam, phi = go.inverse(0.0, 0.0, 7.0, 46.0)
    assert (float(lam), float(phi)) == (float(np.radians(7.0)), float(np.radians(46.0)))
    # forward o inverse is the identity (about one centre), on every finite scene gate
    for name in go.SCENES:
        s = go.scene(name)
        x, y = s.x[s.finite].astype(np.float64), s.y[s.finite].astype(np.float64)
        bx, by = go.forward(*go.inverse(x, y, *s.radar), *s.radar)
        assert np.abs(bx - x).max() <= 1e-7 and np.abs(by - y).max() <= 1e-7, name


def test_translation_misplaces_gates_by_kilometres():
    """The figures of the issue: radar B 200 km east of A (the RMA1 site); where translation puts three of B's gates
    against where they are.  4 510 m, 4 607 m and 1 919 m."""
    s = go.scene("east_200km")
    gates = np.array([[0.0, 2.4e5], [2.4e5, 0.0], [-1.0e5, 0.0]], dtype=np.float32)
    x, y, (ox, oy) = go.place(gates[:, 0], gates[:, 1], s.radar, s.origin)
    off = np.hypot(x - gates[:, 0], y - gates[:, 1])              # placed (relative to the antenna) against untouched
    assert abs(ox - 2.0e5) < 1e-6 and abs(oy) < 1e-6
    assert off[0] > 4000.0 and off[1] > 4000.0 and off[2] > 1500.0
    assert np.allclose(off, [4509.9, 4607.3, 1918.6], atol=0.5)
    # ... and the host maps say the same
    lon, lat = rg.grid_to_geographic(gates[:, 0], gates[:, 1], *s.radar)
    hx, hy = rg.geographic_to_grid(lon, lat, *s.origin)
    assert np.abs(hx - ox - x).max() < 1e-6 and np.abs(hy - oy - y).max() < 1e-6


def test_antimeridian_scene_is_continuous():
    """Origin at lon 179.9, radar at -179.9: the radar lies 0.2 degrees EAST of the origin, not 359.8 west, and its gates
    are placed about as far from the untouched ones as at any other longitude."""
    s = go.scene("antimeridian")
    x, y, (ox, oy) = go.place(s.x, s.y, s.radar, s.origin)
    assert 0.0 < ox < 30e3 and -60e3 < oy < -50e3
    fin = s.finite
    shift = np.hypot(x[fin] - s.x[fin], y[fin] - s.y[fin])
    assert shift.max() < 5e3
    # the same placement moved 90 degrees of longitude away from the antimeridian gives the same plane coordinates
    x2, y2, (ox2, oy2) = go.place(s.x, s.y, (s.radar[0] + 360.0 - 90.0, s.radar[1]), (s.origin[0] - 90.0, s.origin[1]))
    assert abs(ox - ox2) < 1e-6 and abs(oy - oy2) < 1e-6
    assert np.nanmax(np.abs(x - x2)) < 1e-6 and np.nanmax(np.abs(y - y2)) < 1e-6
    lon, _ = rg.grid_to_geographic(np.array([-30e3, 0.0, 30e3]), np.zeros(3), *s.origin)
    assert np.all((lon >= -180.0) & (lon < 180.0)) and lon[0] > 179.0 and lon[2] < -179.0


# ---- the host maps ---------------------------------------------------------------------------------------------------------
def test_host_maps_against_40_digits():
    mp = go._mp()
    for name in ("east_200km", "antimeridian", "lat_80", "equator", "north_mid"):
        s = go.scene(name)
        pick = np.nonzero(s.finite)[0][:120]
        x, y = s.x[pick].astype(np.float64), s.y[pick].astype(np.float64)
        lon, lat = rg.grid_to_geographic(x, y, *s.radar)
        assert lon.dtype == lat.dtype == np.float64 and np.all((lon >= -180.0) & (lon < 180.0))
        hx, hy = rg.geographic_to_grid(lon, lat, *s.origin)
        worst_inv = worst_fwd = 0.0
        for i in range(len(pick)):
            # inverse: its lon / lat, mapped forward about the SAME centre at 40 digits, must be the point it started from
            bx, by = go.mp_forward(mp.radians(mp.mpf(float(lon[i]))), mp.radians(mp.mpf(float(lat[i]))), *s.radar)
            worst_inv = max(worst_inv, abs(float(bx - mp.mpf(float(x[i])))), abs(float(by - mp.mpf(float(y[i])))))
            fx, fy = go.mp_forward(mp.radians(mp.mpf(float(lon[i]))), mp.radians(mp.mpf(float(lat[i]))), *s.origin)
            worst_fwd = max(worst_fwd, abs(float(fx - mp.mpf(float(hx[i])))), abs(float(fy - mp.mpf(float(hy[i])))))
        print(f"{name}: host inverse {worst_inv:.3g} m, host forward {worst_fwd:.3g} m")
        assert worst_inv <= HOST_BOUND_M and worst_fwd <= HOST_BOUND_M, name
    assert rg.geographic_to_grid(7.0, 46.0, 7.0, 46.0) == (0.0, 0.0)
    lon, lat = rg.grid_to_geographic(0.0, 0.0, 7.0, 46.0)
    assert abs(float(lon) - 7.0) < 1e-13 and abs(float(lat) - 46.0) < 1e-13
    assert rg.AEQD_EARTH_RADIUS == go.R_EARTH == 6370997.0


def test_make_georef_holds_what_the_host_maps_give():
    s = go.scene("north_mid")
    g = georef.make_georef(s.radar, s.origin)
    ox, oy = rg.geographic_to_grid(*s.radar, *s.origin)
    assert (g.ox, g.oy, g.same_centre) == (float(ox), float(oy), 0) and g.radius == rg.AEQD_EARTH_RADIUS
    assert g.lon_from == float(np.radians(s.radar[0])) and g.lat_to == float(np.radians(s.origin[1]))
    assert g.sin_lat_from == float(np.sin(g.lat_from)) and g.cos_lat_to == float(np.cos(g.lat_to))
    same = georef.make_georef(s.origin + (812.0,), s.origin)                 # an altitude is ignored
    assert (same.ox, same.oy, same.same_centre) == (0.0, 0.0, 1)


def test_section_path_lonlat_is_section_path_of_the_mapped_vertices():
    origin = (-64.19, -31.44, 400.0)
    vertices = [(-62.5, -29.4), (-62.0, -29.2), (-61.9, -29.5)]
    xs, ys, s = rg.section_path_lonlat(vertices, 750.0, origin)
    vx, vy = rg.geographic_to_grid([v[0] for v in vertices], [v[1] for v in vertices], origin[0], origin[1])
    want = rg.section_path(np.stack([vx, vy], axis=1), 750.0)
    assert all(np.array_equal(a, b) for a, b in zip((xs, ys, s), want)) and xs.dtype == np.float32
    assert rg.section_path_lonlat(vertices, 750.0, origin[:2])[0].tobytes() == xs.tobytes()


# ---- refusals: all before any device call ----------------------------------------------------------------------------------
def test_every_refusal_raises_without_a_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_native, "load_library", no_device)
    monkeypatch.setattr(_native, "canonical_device", no_device)
    x = np.zeros(4, dtype=np.float32)
    ok, origin = (10.0, 45.0), (11.0, 45.5)
    far = (10.0 + math.degrees(math.pi / 2 - 0.1) + 0.01, 0.0)               # on the equator, just past the limit from (10, 0)
    near = (10.0 + math.degrees(math.pi / 2 - 0.1) - 0.01, 0.0)
    for bad in ((10.0, 90.5), (10.0, -91.0), (np.nan, 45.0), (10.0, np.inf)):
        with pytest.raises(ValueError):
            rg.place_gates_device(x, x, bad, origin)
        with pytest.raises(ValueError):
            rg.place_gates_device(x, x, ok, bad)
        with pytest.raises(ValueError):
            rg.place_radar(x, x, x, bad + (0.0,), origin + (0.0,))
        with pytest.raises(ValueError):
            rg.geographic_to_grid(*bad, *origin)
        with pytest.raises(ValueError):
            rg.geographic_to_grid(*ok, *bad)
        with pytest.raises(ValueError):
            rg.grid_to_geographic(0.0, 0.0, *bad)
        with pytest.raises(ValueError):
            rg.grid_lonlat_device((2, 3, 4), ((0, 1), (0, 1), (0, 1)), bad)
        with pytest.raises(ValueError):
            rg.section_path_lonlat([ok, origin], 100.0, bad)
    with pytest.raises(ValueError, match="finite"):
        rg.place_radar(x, x, x, ok + (np.nan,), origin + (0.0,))            # a non-finite altitude
    with pytest.raises(ValueError, match="lon, lat, alt"):
        rg.place_radar(x, x, x, ok, origin + (0.0,))                         # no altitude
    for bad_r in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="R must be finite and positive"):
            rg.place_gates_device(x, x, ok, origin, R=bad_r)
        with pytest.raises(ValueError, match="R must be finite and positive"):
            rg.geographic_to_grid(*ok, *origin, R=bad_r)
        with pytest.raises(ValueError, match="R must be finite and positive"):
            rg.grid_to_geographic(1.0, 2.0, *origin, R=bad_r)
        with pytest.raises(ValueError, match="R must be finite and positive"):
            rg.grid_lonlat_device((2, 3, 4), ((0, 1), (0, 1), (0, 1)), origin, R=bad_r)
    with pytest.raises(ValueError, match="differ in length"):
        rg.place_gates_device(x, x[:3], ok, origin)
    with pytest.raises(ValueError, match="differ in length"):
        rg.place_radar(x, x, x[:2], ok + (0.0,), origin + (0.0,))
    with pytest.raises(ValueError, match="out must be two tensors"):
        rg.place_gates_device(x, x, ok, origin, out=(x[:3], x))
    # the angular-distance limit: pi/2 - 0.1 rad or more from the origin
    with pytest.raises(ValueError, match="rad from the origin"):
        rg.place_gates_device(x, x, far, (10.0, 0.0))
    with pytest.raises(ValueError, match="rad from the origin"):
        rg.place_radar(x, x, x, far + (0.0,), (10.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="rad from the origin"):
        rg.geographic_to_grid(*far, 10.0, 0.0)
    with pytest.raises(ValueError, match="rad from the origin"):
        rg.geographic_to_grid([10.5, far[0]], [0.0, 0.0], 10.0, 0.0)
    with pytest.raises(ValueError, match="rad from the origin"):
        rg.section_path_lonlat([(10.5, 0.0), far], 100.0, (10.0, 0.0))
    gx, gy = rg.geographic_to_grid(*near, 10.0, 0.0)                         # just inside: accepted
    assert abs(float(gx) / rg.AEQD_EARTH_RADIUS - (math.pi / 2 - 0.1 - math.radians(0.01))) < 1e-12 and abs(float(gy)) < 1e-6
    with pytest.raises(ValueError, match="at least two"):
        rg.section_path_lonlat([ok], 100.0, origin)
    with pytest.raises(ValueError, match="bad grid shape"):
        rg.grid_lonlat_device((2, 0, 4), ((0, 1), (0, 1), (0, 1)), origin)

    class Radar:
        gate_x = gate_y = gate_z = {"data": np.zeros((2, 2))}
        longitude, latitude, altitude = {"data": [10.0]}, {"data": [95.0]}, {"data": [100.0]}
    with pytest.raises(ValueError, match="latitude"):
        rg.place_radars([Radar()], origin + (0.0,))


def test_entry_points_refuse_bad_arguments_without_a_device():
    lib = rg.load_library(require_device=False)
    s = go.scene("north_mid")
    good = georef.make_georef(s.radar, s.origin)
    A, B, C, D = P, 2 * P, 3 * P, 4 * P                # four arrays of up to 1024 floats that do not overlap

    def gates(x=A, y=B, n=16, g=good, xo=C, yo=D):
        return lib.rg_gates_to_frame_f32(x, y, n, g, xo, yo, None)

    def lonlat(xc=A, yc=B, ny=4, nx=5, g=good, lon=C, lat=D):
        return lib.rg_frame_to_lonlat_f64(xc, yc, ny, nx, g, lon, lat, None)

    def refused(status, word):
        assert status == _native.RG_EINVAL
        msg = lib.rg_last_error()
        assert word in msg, msg

    for kw in (dict(x=None), dict(y=None), dict(g=None), dict(xo=None), dict(yo=None)):
        refused(gates(**kw), b"rg_gates_to_frame_f32: null")
    for kw in (dict(xc=None), dict(yc=None), dict(g=None), dict(lon=None), dict(lat=None)):
        refused(lonlat(**kw), b"rg_frame_to_lonlat_f64: null")
    refused(gates(n=-1), b"rg_gates_to_frame_f32: negative")
    refused(lonlat(ny=-1), b"rg_frame_to_lonlat_f64: negative")
    refused(lonlat(nx=-3), b"rg_frame_to_lonlat_f64: negative")
    for name, _ in _native.Georef._fields_[:-2]:
        for bad in (math.nan, math.inf) + ((0.0, -6370997.0) if name == "radius" else ()):
            g = georef.make_georef(s.radar, s.origin)
            setattr(g, name, bad)
            refused(gates(g=g), b"rg_gates_to_frame_f32: ")
            refused(lonlat(g=g), b"rg_frame_to_lonlat_f64: ")
            assert (b"radius" if name == "radius" else b"not finite") in lib.rg_last_error()
    g = georef.make_georef(s.radar, s.origin)
    g.same_centre = 7
    refused(gates(g=g), b"same_centre")
    # arrays that overlap without being the same array; the same array as input and output is the in-place call
    refused(gates(xo=A + 8), b"overlaps")
    refused(gates(yo=B - 4), b"overlaps")
    refused(gates(xo=C, yo=C), b"x_out and y_out")
    refused(gates(xo=C, yo=C + 32), b"x_out and y_out")
    refused(lonlat(lat=C), b"lon and lat")
    refused(lonlat(lat=C + 8), b"lon and lat")
    # nothing to do: RG_OK without a launch (no device here), null-free but never dereferenced
    assert gates(n=0) == _native.RG_OK and gates(n=0, xo=A, yo=B) == _native.RG_OK
    assert lonlat(ny=0) == _native.RG_OK and lonlat(nx=0) == _native.RG_OK


# ---- bookkeeping -----------------------------------------------------------------------------------------------------------
def test_abi_bookkeeping_and_exports():
    header = open(os.path.join(REPO, "include", "radargrid_hip.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t|const char\*)\s+(rg_\w+)\s*\(", header, flags=re.M))
    for name in ("rg_gates_to_frame_f32", "rg_frame_to_lonlat_f64"):
        assert name in declared and name in _native.SIGNATURES
    assert "#define RG_VERSION 104" in header and _native.ABI_VERSION == 104
    body = re.search(r"typedef struct rg_georef \{(.*?)\} rg_georef;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [m.strip() for decl in re.findall(r"(?:double|int32_t)\s+([^;]+);", body) for m in decl.split(",")]
    assert members == [name for name, _ in _native.Georef._fields_]
    from radar_processor_amd import build
    assert ("rg_georef.hip", []) in build.SOURCES
    for name in ("AEQD_EARTH_RADIUS", "geographic_to_grid", "grid_to_geographic", "place_gates_device", "place_radar",
                 "place_radars", "section_path_lonlat", "grid_lonlat_device"):
        assert name in rg.__all__ and getattr(rg, name) is getattr(georef, name)
    from radar_processor_amd import mosaic
    assert "place_radar" in mosaic.__doc__
