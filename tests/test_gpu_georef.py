"""Georeferencing on the GPU: ``rg_gates_to_frame_f32`` and ``rg_frame_to_lonlat_f64`` against the float64 / 40-digit
restatements of tests/georef_oracle.py on every gate of every scene, their special cases and memory discipline, the tuple
``place_radar`` makes, and the physical point of it all: two radars 200 km apart see one target in ONE voxel once they are
placed by longitude and latitude, and 4.5 km apart when they are only translated.

The bound of the kernel test is ``|got - float32(want)| <= ulp_f32(want) + 1e-6 m``.  The micrometre is derived: one
float64 rounding at the earth's radius is 6.4e6 * 1.1e-16 = 7e-10 m; the floor allows about a thousand of them plus the
restatement's own distance from the 40-digit value (profiles/georef_bounds.json: under 1e-8 m).  It matters only where an
output is near zero (a float32 ulp is then smaller than float64 noise at the earth's radius)."""
import json

import numpy as np
import pytest

import georef_oracle as go

pytestmark = pytest.mark.gpu
CANARY = 64                       # floats (or doubles) before and after every output
LONLAT_BOUND_M = 1e-6


@pytest.fixture(scope="module")
def env():
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native, georef
    lib = rg.load_library()
    return dict(torch=torch, rg=rg, native=_native, georef=georef, lib=lib, dev=torch.device("cuda", 0))


def _guarded(env, n, dtype, pattern):
    """A buffer of CANARY + n + CANARY elements filled with ``pattern``; returns (buffer, view of the n in the middle)."""
    buf = env["torch"].full((n + 2 * CANARY,), pattern, dtype=dtype, device=env["dev"])
    return buf, buf[CANARY:CANARY + n]


def _canaries_intact(buf, n, pattern):
    host = buf.cpu().numpy()
    return bool((host[:CANARY] == pattern).all() and (host[CANARY + n:] == pattern).all())


def _gates_call(env, georef, x_t, y_t, xo_t, yo_t, n):
    nat = env["native"]
    with env["torch"].cuda.device(env["dev"]):
        nat.check(env["lib"].rg_gates_to_frame_f32(nat.ptr(x_t), nat.ptr(y_t), n, georef, nat.ptr(xo_t), nat.ptr(yo_t),
                                                   nat.stream_ptr()), "rg_gates_to_frame_f32")


# ---- the gate kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", go.SCENES)
def test_kernel_against_the_float64_restatement_on_every_gate(env, name):
    d = go.kernel_differences(name, env["dev"])
    print(f"{name}: {json.dumps(d)}")
    assert d["values"] == 2 * int(go.scene(name).finite.sum())
    assert d["nonfinite_as_contract"]
    assert d["worst_excess_m"] <= 0.0, f"{name}: a value lies {d['worst_excess_m']} m beyond ulp_f32(want) + 1e-6 m"
    if name == "at_origin":
        assert d["values_differing"] == 0


def test_same_centre_copies_bit_for_bit_and_nonfinite_gates_give_nan(env):
    torch, rg = env["torch"], env["rg"]
    s = go.scene("at_origin")
    assert s.radar == s.origin and (~s.finite).sum() == go.N_NONFINITE
    x, y = rg.place_gates_device(s.x, s.y, s.radar, s.origin, device=env["dev"])
    assert x.dtype == y.dtype == torch.float32 and x.device == env["dev"]
    assert x.cpu().numpy().tobytes() == s.x.tobytes() and y.cpu().numpy().tobytes() == s.y.tobytes()   # NaN and inf included
    for name in ("east_1m", "lat_80"):
        s = go.scene(name)
        x, y = (t.cpu().numpy() for t in rg.place_gates_device(s.x, s.y, s.radar, s.origin, device=env["dev"]))
        assert np.isnan(x[~s.finite]).all() and np.isnan(y[~s.finite]).all()
        assert np.isfinite(x[s.finite]).all() and np.isfinite(y[s.finite]).all()
        at_antenna = s.finite & (s.x == 0) & (s.y == 0)
        assert at_antenna.sum() >= 180 and not x[at_antenna].any() and not y[at_antenna].any()     # rho == 0: exactly (0, 0)


@pytest.mark.parametrize("n", go.LENGTHS)
def test_canaries_and_in_place_at_every_length(env, n):
    torch = env["torch"]
    s = go.scene("east_200km")
    assert s.x.size >= n
    georef = env["georef"].make_georef(s.radar, s.origin)
    x_t, y_t = torch.from_numpy(s.x[:n].copy()).to(env["dev"]), torch.from_numpy(s.y[:n].copy()).to(env["dev"])
    pattern = np.float32(-12345.5)
    bx, xo = _guarded(env, n, torch.float32, float(pattern))
    by, yo = _guarded(env, n, torch.float32, float(pattern))
    _gates_call(env, georef, x_t, y_t, xo, yo, n)
    torch.cuda.synchronize()
    assert _canaries_intact(bx, n, pattern) and _canaries_intact(by, n, pattern)
    assert x_t.cpu().numpy().tobytes() == s.x[:n].tobytes() and y_t.cpu().numpy().tobytes() == s.y[:n].tobytes()   # inputs untouched
    # against the restatement, this prefix
    want = [w[:n] for w in go.placed("east_200km")]
    fin = s.finite[:n]
    for got, w in zip((xo.cpu().numpy(), yo.cpu().numpy()), want):
        assert np.isnan(got[~fin]).all()
        assert (np.abs(got[fin].astype(np.float64) - w[fin].astype(np.float32)) <= go.ulp_f32(w[fin]) + go.KERNEL_FLOOR_M).all()
    # in place (x_out is x, y_out is y), inside guarded buffers: the same bits, the canaries unchanged
    bix, xi = _guarded(env, n, torch.float32, float(pattern))
    biy, yi = _guarded(env, n, torch.float32, float(pattern))
    xi.copy_(x_t)
    yi.copy_(y_t)
    _gates_call(env, georef, xi, yi, xi, yi, n)
    torch.cuda.synchronize()
    assert _canaries_intact(bix, n, pattern) and _canaries_intact(biy, n, pattern)
    assert torch.equal(xi.view(torch.int32), xo.view(torch.int32)) and torch.equal(yi.view(torch.int32), yo.view(torch.int32))
    # ... and through the Python surface: out= the input tensors themselves
    px, py = env["rg"].place_gates_device(x_t, y_t, s.radar, s.origin, out=(x_t, y_t))
    assert px.data_ptr() == x_t.data_ptr() and py.data_ptr() == y_t.data_ptr()
    assert torch.equal(px.view(torch.int32), xo.view(torch.int32)) and torch.equal(py.view(torch.int32), yo.view(torch.int32))


# ---- place_radar -----------------------------------------------------------------------------------------------------------
def test_place_radar_returns_the_tuple_the_mosaic_takes(env, tmp_path):
    rg = env["rg"]
    from radar_processor_amd import synthetic
    vol = synthetic.make_volume(n_elev=3, n_az=72, n_gates=60, seed=5, fields=("DBZH",))
    s = go.scene("north_mid")
    radar, origin = s.radar + (512.0,), s.origin + (87.5,)
    x, y, z, o = rg.place_radar(vol.gate_x, vol.gate_y, vol.gate_z, radar, origin, device=env["dev"])
    assert z is vol.gate_z
    ox, oy = rg.geographic_to_grid(*s.radar, *s.origin)
    assert o == (512.0 - 87.5, float(oy), float(ox))
    want = go.place(vol.gate_x, vol.gate_y, s.radar, s.origin)
    for got, w in zip((x.cpu().numpy(), y.cpu().numpy()), want[:2]):
        assert (np.abs(got.astype(np.float64) - w.astype(np.float32)) <= go.ulp_f32(w) + go.KERNEL_FLOOR_M).all()
    assert abs(want[2][0] - float(ox)) < 1e-6 and abs(want[2][1] - float(oy)) < 1e-6

    # a radar standing at the origin: the tuple's mosaic geometry is today's, array for array
    here = origin[:2] + (origin[2] + 0.0,)
    placed = rg.place_radar(vol.gate_x, vol.gate_y, vol.gate_z, here, origin, device=env["dev"])
    assert placed[3] == (0.0, 0.0, 0.0)
    shape, limits = (4, 18, 20), ((500.0, 6500.0), (-40e3, 45e3), (-50e3, 38e3))
    a = rg.compute_mosaic_geometry([placed], shape, limits, str(tmp_path), min_radius=3000.0)
    b = rg.compute_mosaic_geometry([(vol.gate_x, vol.gate_y, vol.gate_z, (0.0, 0.0, 0.0))], shape, limits, str(tmp_path),
                                   min_radius=3000.0)
    assert b.n_pairs() > 1000
    for name in ("indptr", "gate_indices", "weights"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name

    # place_radars: duck-typed PyART radars
    class Radar:
        def __init__(self, pos):
            self.gate_x, self.gate_y, self.gate_z = ({"data": c.reshape(3 * 72, 60)} for c in (vol.gate_x, vol.gate_y, vol.gate_z))
            self.longitude, self.latitude, self.altitude = ({"data": np.array([v])} for v in pos)
    many = rg.place_radars([Radar(radar), Radar(here)], origin, device=env["dev"])
    assert len(many) == 2 and many[0][3] == o and many[1][3] == (0.0, 0.0, 0.0)
    assert env["torch"].equal(many[0][0].view(env["torch"].int32), x.view(env["torch"].int32))
    assert np.array_equal(many[0][2], vol.gate_z) and many[0][2].dtype == np.float32


# ---- the node kernel -------------------------------------------------------------------------------------------------------
ORIGINS = sorted({go.PLACEMENTS[name][1] for name in go.SCENES})


@pytest.mark.parametrize("origin", ORIGINS, ids=[f"{o[0]}_{o[1]}" for o in ORIGINS])
def test_node_lonlat_against_40_digits(env, origin):
    torch, nat = env["torch"], env["native"]
    ny, nx = 33, 47
    shape, limits = (2, ny, nx), ((0.0, 1000.0), (-310e3, 255e3), (-401e3, 377e3))
    lon_t, lat_t = env["rg"].grid_lonlat_device(shape, limits, origin, device=env["dev"])
    assert lon_t.shape == lat_t.shape == (ny, nx) and lon_t.dtype == lat_t.dtype == torch.float64
    lon, lat = lon_t.cpu().numpy(), lat_t.cpu().numpy()
    assert ((lon >= -180.0) & (lon < 180.0)).all() and (np.abs(lat) <= 90.0).all()
    if origin[0] > 179.0:
        assert (lon < 0).any() and (lon > 0).any()                # the grid straddles the antimeridian
    yc = np.linspace(limits[1][0], limits[1][1], ny, dtype="float32")
    xc = np.linspace(limits[2][0], limits[2][1], nx, dtype="float32")
    mp = go._mp()
    worst = 0.0
    for iy in range(ny):
        for ix in range(nx):
            bx, by = go.mp_forward(mp.radians(mp.mpf(float(lon[iy, ix]))), mp.radians(mp.mpf(float(lat[iy, ix]))), *origin)
            worst = max(worst, abs(float(bx - mp.mpf(float(xc[ix])))), abs(float(by - mp.mpf(float(yc[iy])))))
    print(f"origin {origin}: kernel lon/lat mapped forward at 40 digits lies {worst:.3g} m from the node at worst")
    assert worst <= LONLAT_BOUND_M
    # the host map agrees (degrees; 1e-11 degrees is a micrometre on the ground)
    h_lon, h_lat = env["rg"].grid_to_geographic(xc[None, :].astype(np.float64), yc[:, None].astype(np.float64), *origin)
    d_lon = np.abs(lon - h_lon)
    assert np.minimum(d_lon, 360.0 - d_lon).max() < 1e-10 and np.abs(lat - h_lat).max() < 1e-11

    # canaries around both planes, through the C entry point; a table entry that is not finite gives NaN in both
    georef = env["georef"].make_georef(origin, origin)
    pattern = -98765.25
    b_lon, o_lon = _guarded(env, ny * nx, torch.float64, pattern)
    b_lat, o_lat = _guarded(env, ny * nx, torch.float64, pattern)
    xc_bad = xc.copy()
    xc_bad[5] = np.nan
    xc_t, yc_t = torch.from_numpy(xc_bad).to(env["dev"]), torch.from_numpy(yc).to(env["dev"])
    with torch.cuda.device(env["dev"]):
        nat.check(env["lib"].rg_frame_to_lonlat_f64(nat.ptr(xc_t), nat.ptr(yc_t), ny, nx, georef, nat.ptr(o_lon),
                                                    nat.ptr(o_lat), nat.stream_ptr()), "rg_frame_to_lonlat_f64")
    torch.cuda.synchronize()
    assert _canaries_intact(b_lon, ny * nx, pattern) and _canaries_intact(b_lat, ny * nx, pattern)
    g_lon, g_lat = o_lon.cpu().numpy().reshape(ny, nx), o_lat.cpu().numpy().reshape(ny, nx)
    assert np.isnan(g_lon[:, 5]).all() and np.isnan(g_lat[:, 5]).all()
    keep = np.arange(nx) != 5
    assert np.array_equal(g_lon[:, keep], lon[:, keep]) and np.array_equal(g_lat[:, keep], lat[:, keep])


# ---- the physical test -----------------------------------------------------------------------------------------------------
N_SWEEPS, N_RAYS, N_GATES = 3, 72, 60
TARGET = (1 * N_RAYS + 7) * N_GATES + 59           # the gate of each radar that is moved onto the target
SHAPE = (3, 48, 48)
MIN_RADIUS = 800.0      # > 707 m: a gate at a level is within it of some node of a 1 km lattice; < 1 km: of one node only
                        # when it sits on a node


def _volume():
    """3 sweeps x 72 rays x 60 gates to 150 km: float32 x, y, z relative to the antenna, flat, ray-major."""
    el = np.radians([0.5, 1.5, 2.5])[:, None, None]
    az = np.radians(np.arange(N_RAYS) * 5.0)[None, :, None]
    r = ((np.arange(N_GATES) + 1) * 2500.0)[None, None, :]
    x, y = r * np.cos(el) * np.sin(az), r * np.cos(el) * np.cos(az)
    z = r * np.sin(el) + r * r / (2.0 * 4.0 / 3.0 * go.R_EARTH) + 0.0 * az
    return tuple(np.ascontiguousarray(np.broadcast_to(c, (N_SWEEPS, N_RAYS, N_GATES)), dtype=np.float32).ravel() for c in (x, y, z))


@pytest.fixture(scope="module")
def two_radars():
    """Radar A at the grid origin (RMA1, 400 m), radar B 200 km east of it (500 m); one gate of each moved, by the oracle's
    maps, onto the geographic point 240 km north of B, 4 000 m above the grid origin's altitude."""
    A, B = go.RMA1 + (400.0,), go.PLACEMENTS["east_200km"][0] + (500.0,)
    lam, phi = go.inverse(0.0, 2.4e5, *B[:2])
    xa, ya = (float(v) for v in go.forward(lam, phi, *A[:2]))
    ox, oy = (float(v) for v in go.forward(*np.radians(B[:2]), *A[:2]))
    gates = {}
    for key, (tx, ty, tz) in (("A", (xa, ya, 4000.0)), ("B", (0.0, 2.4e5, 4000.0 - 100.0))):
        x, y, z = (c.copy() for c in _volume())
        x[TARGET], y[TARGET], z[TARGET] = tx, ty, tz
        gates[key] = (x, y, z)
    # node (iz 1, iy 24, ix 24) of the grid is the target
    limits = ((3000.0, 5000.0), (ya - 24e3, ya + 23e3), (xa - 24e3, xa + 23e3))
    n = N_SWEEPS * N_RAYS * N_GATES
    values = {"A": np.arange(n, dtype=np.float32), "B": 20000.0 + np.arange(n, dtype=np.float32)}
    both = (values["A"][TARGET] + values["B"][TARGET]) / np.float32(2.0)
    return dict(A=A, B=B, gates=gates, limits=limits, values=values, both=both, xa=xa, ya=ya,
                translated=[gates["A"] + ((0.0, 0.0, 0.0),), gates["B"] + ((100.0, oy, ox),)])


def _placed(env, t):
    rg = env["rg"]
    return [rg.place_radar(*t["gates"][k], t[k], t["A"], device=env["dev"]) for k in ("A", "B")]


def _device_fields(env, t):
    return [[env["torch"].from_numpy(t["values"][k]).to(env["dev"])] for k in ("A", "B")]


def _filled(grid):
    return sorted(zip(*(int_idx.tolist() for int_idx in np.nonzero(np.isfinite(grid)))))


def test_one_target_two_radars_one_voxel(env, two_radars, tmp_path):
    rg, t = env["rg"], two_radars
    kw = dict(min_radius=MIN_RADIUS, beam_factor=0.0)
    fields = _device_fields(env, t)

    # placed by longitude and latitude: both target gates are neighbours of ONE voxel, the node they were planted on
    placed = _placed(env, t)
    search = rg.MosaicSearch(placed, SHAPE, t["limits"], device=env["dev"], **kw)
    grid = rg.mosaic_fields_device(search, fields, weighting="nearest", combine="mean")[0].cpu().numpy()
    assert _filled(grid) == [(1, 24, 24)]
    assert grid[1, 24, 24] == t["both"]

    # translated only (today's tuples): each radar fills voxels of its own, at least 4 voxels apart, none with the mean
    search_t = rg.MosaicSearch(t["translated"], SHAPE, t["limits"], device=env["dev"], **kw)
    grid_t = rg.mosaic_fields_device(search_t, fields, weighting="nearest", combine="mean")[0].cpu().numpy()
    of_a = [v for v in _filled(grid_t) if grid_t[v] == t["values"]["A"][TARGET]]
    of_b = [v for v in _filled(grid_t) if grid_t[v] == t["values"]["B"][TARGET]]
    assert of_a == [(1, 24, 24)] and of_b and len(of_a) + len(of_b) == len(_filled(grid_t))
    assert not (grid_t == t["both"]).any()
    apart = min(float(np.linalg.norm(np.subtract(a, b))) for a in of_a for b in of_b)
    print(f"translated: radar B's target fills {of_b}, {apart:.2f} voxels from radar A's at the nearest")
    assert apart >= 4.0

    # the placed case through a mosaic geometry: the row of the common voxel holds exactly the two target gates
    geom = rg.compute_mosaic_geometry(placed, SHAPE, t["limits"], str(tmp_path), weighting="nearest", **kw)
    n = N_SWEEPS * N_RAYS * N_GATES
    row = (1 * SHAPE[1] + 24) * SHAPE[2] + 24
    assert geom.n_pairs() == 2
    assert sorted(geom.gate_indices[geom.indptr[row]:geom.indptr[row + 1]].tolist()) == [TARGET, n + TARGET]
    host = [np.ma.masked_invalid(t["values"][k]) for k in ("A", "B")]
    via_geom = rg.apply_mosaic(geom, host)
    assert _filled(via_geom) == [(1, 24, 24)] and via_geom[1, 24, 24] == t["both"]

    # ... and through a section across the target, its path given by geographic vertices
    # (10 km to either side of the target along the direction (0.8, 0.6): sample 10 of 1 km steps is the target)
    lon, lat = rg.grid_to_geographic(np.array([t["xa"] - 8e3, t["xa"] + 8e3]), np.array([t["ya"] - 6e3, t["ya"] + 6e3]),
                                     *t["A"][:2])
    xs, ys, s = rg.section_path_lonlat(list(zip(lon, lat)), 1000.0, t["A"])
    assert xs.size == 21 or xs.size == 20
    assert abs(float(xs[10]) - t["xa"]) < 0.05 and abs(float(ys[10]) - t["ya"]) < 0.05
    path = rg.MosaicSearch.for_path(placed, xs, ys, t["limits"][0], SHAPE[0], device=env["dev"], **kw)
    sec = rg.mosaic_section_fields_device(path, xs, ys, fields, weighting="nearest", combine="mean")[0].cpu().numpy()
    assert sec.shape == (SHAPE[0], xs.size)
    assert _filled(sec) == [(1, 10)] and sec[1, 10] == t["both"]
    path_t = rg.MosaicSearch.for_path(t["translated"], xs, ys, t["limits"][0], SHAPE[0], device=env["dev"], **kw)
    sec_t = rg.mosaic_section_fields_device(path_t, xs, ys, fields, weighting="nearest", combine="mean")[0].cpu().numpy()
    assert not (sec_t == t["both"]).any() and sec_t[1, 10] == t["values"]["A"][TARGET]
