"""Echo top, echo base and VIL on the MI355X (``rg_column_profile_f32``) against the float64 restatement of the contract
(tests/column_profile_oracle.py), through the public functions and the C ABI.

 1. Kernel: nz in {1, 2, 7, 40} crossed with a single column, the one-column path (15 columns), the vector path (256
    columns), each also with more than one block, an unaligned grid pointer and unaligned output planes; constructed
    columns for every case of the contract next to seeded random ones (0.5 dB lattice in -10 .. 70, 30 % NaN); the full window, a one-level window and interior
    windows by index and by altitude.  Echo planes are bit-identical to the restatement, ``nearest`` planes hold level
    heights only, VIL has the restatement's NaN pattern and is within one float32 ulp of it elsewhere (the device's float64
    exp10 / log2 / exp2 and the <= 40-term float64 sum err by ~1e-14 relative against a float32 half-ulp of 6e-8, so the two
    roundings can only differ at a rounding boundary).  The largest VIL difference seen, in ulp, is printed and written to
    column_profile_bounds.json where RG_REPORT_DIR names a directory.
 2. Independence: four thresholds in one launch against four launches of one; ``column_profile`` with everything against
    the three named functions; the vector against the one-column path on the same columns.
 3. Routes: ``PlaneProducts(echo_top=..., echo_base=..., vil=True)`` through ``grid_products_device`` on a CSR geometry, a
    two-radar ``MosaicSearch`` (``combine`` mean and max) and ``VolumeBatch.grid_shard`` on a CSR geometry and on a
    ``RoiSearch`` returns, bit for bit, what ``column_profile`` gives on the grid the same route returns without
    ``products``; the other keys of the record are those of a request without the new arguments."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import column_profile_oracle as cpo
import mosaic_scenes

pytestmark = pytest.mark.gpu

T = 18.0                                     # the threshold the constructed columns are built around
THRESHOLDS = (18.0, 30.0, 45.0, -3.5)
NZS = (1, 2, 7, 40)
SHAPES = {"one": (1, 1), "scalar": (3, 5), "vector": (4, 64),
          "scalar_blocks": (7, 43), "vector_blocks": (8, 160)}        # 301 and 320 lanes: more than one 256-thread block
REPORT = {"vil_max_ulp": 0.0, "vil_planes": 0, "vil_values": 0}
NAN, INF = np.float32(np.nan), np.float32(np.inf)


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
    print("column_profile_bounds", json.dumps(REPORT, sort_keys=True))
    out_dir = os.environ.get("RG_REPORT_DIR")
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "column_profile_bounds.json"), "w") as fh:
            json.dump(REPORT, fh, indent=1, sort_keys=True)


class Geom:
    """Anything with ``grid_shape`` / ``grid_limits``."""

    def __init__(self, shape, z_limits=(500.0, 19750.0)):
        self.grid_shape = tuple(shape)
        self.grid_limits = (tuple(z_limits), (-1e3, 1e3), (-1e3, 1e3))


def levels(geom):
    return np.linspace(geom.grid_limits[0][0], geom.grid_limits[0][1], geom.grid_shape[0])


# ---- columns -----------------------------------------------------------------------------------------------------------------
def constructed_columns(nz, lo, hi):
    """One column per case of the contract, around threshold T and the window ``lo .. hi`` (for tiny nz several coincide)."""
    mid = (lo + hi) // 2
    up, down = min(mid + 1, nz - 1), max(mid - 1, 0)
    cols = []

    def col(fill, **at):
        c = np.full(nz, fill, dtype=np.float32)
        for k, v in at.items():
            c[int(k[1:])] = v
        cols.append(c)
        return c
    col(NAN)                                                                  # all NaN
    col(T - 8)                                                                # all below
    col(T + 8)                                                                # all above
    cols.append(np.linspace(T + 22, T - 17, nz).astype(np.float32))            # one crossing, falling
    cols.append(np.linspace(T - 17, T + 22, nz).astype(np.float32))            # one crossing, rising
    cols.append((T + 9.5 * np.cos(np.arange(nz) * 2.1)).astype(np.float32))    # several crossings
    col(T - 5, **{f"k{mid}": T})                                              # value == T
    c = col(T - 5, **{f"k{mid}": T + 4})                                      # NaN neighbours on both sides
    c[up] = NAN if up != mid else c[up]
    c[down] = NAN if down != mid else c[down]
    for at_k, at_n in ((INF, T - 5), (T + 4, INF), (T + 4, -INF), (-INF, T + 4), (INF, INF)):
        c = col(T - 5, **{f"k{mid}": at_k})                                   # +-inf at k and at the neighbours
        if up != mid:
            c[up] = at_n
        if down != mid:
            c[down] = at_n
    c = col(T - 5, **{f"k{hi}": T + 2, f"k{lo}": T + 1})                      # crossings at the window's ends ...
    if hi + 1 < nz:
        c[hi + 1] = 60.0                                                      # ... with a louder echo just outside
    if lo - 1 >= 0:
        c[lo - 1] = 60.0
    return cols


@functools.lru_cache(maxsize=None)
def grid_for(nz, ny, nx, lo, hi, seed=0):
    """Seeded random columns with the constructed ones written over the first columns (as many as fit)."""
    rng = np.random.default_rng([seed, nz, ny, nx])
    g = (rng.integers(-20, 141, size=(nz, ny * nx)) * 0.5).astype(np.float32)
    g[rng.random((nz, ny * nx)) < 0.3] = NAN
    cols = constructed_columns(nz, lo, hi)
    if ny * nx == 1:
        cols = [cols[(3 + nz + lo) % len(cols)]]
    for j, c in enumerate(cols[:ny * nx]):
        g[:, j] = c
    g.setflags(write=False)
    return g.reshape(nz, ny, nx)


def windows(nz):
    """``(lo, hi, keyword arguments)``: the full range, one level, an interior window by index and one by altitude."""
    geom = Geom((nz, 1, 1))
    z = levels(geom)
    out = [(0, nz - 1, {})]
    one = nz // 2
    out.append((one, one, dict(z_min_idx=one, z_max_idx=one)))
    lo, hi = (1, nz - 2) if nz >= 3 else (0, nz - 1)
    out.append((lo, hi, dict(z_min_idx=lo, z_max_idx=hi)))
    if nz >= 3:                                                               # altitudes strictly between levels
        out.append((lo, hi, dict(z_min_alt=float(z[lo] - 1.0), z_max_alt=float(z[hi] + 1.0))))
    seen, uniq = set(), []
    for w in out:
        key = (w[0], w[1], tuple(sorted(w[2])))
        if key not in seen:
            seen.add(key)
            uniq.append(w)
    return uniq


# ---- comparisons -------------------------------------------------------------------------------------------------------------
def host(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def assert_bits(got, want, label):
    got, want = host(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, label
    bad = np.flatnonzero(got.view(np.int32).ravel() != want.view(np.int32).ravel())
    assert bad.size == 0, (label, bad[:8], got.ravel()[bad[:8]], want.ravel()[bad[:8]])


def assert_vil(got, want, label):
    """The NaN pattern of the restatement; elsewhere within one float32 ulp of its value."""
    got, want = host(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, label
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=str(label))
    m = ~np.isnan(want)
    REPORT["vil_planes"] += 1
    if not m.any():
        return
    ulp = np.spacing(np.abs(want[m])).astype(np.float64)
    diff = np.abs(got[m].astype(np.float64) - want[m].astype(np.float64)) / ulp
    worst = float(diff.max())
    print("vil", label, "max ulp", worst, "values", int(m.sum()))
    REPORT["vil_max_ulp"] = max(REPORT["vil_max_ulp"], worst)
    REPORT["vil_values"] += int(m.sum())
    assert worst <= 1.0, (label, worst)


@functools.lru_cache(maxsize=None)
def want_planes(nz, ny, nx, lo, hi, linear):
    """The restatement's planes of ``grid_for(nz, ny, nx, lo, hi)``: computed once, shared by the tests."""
    g = grid_for(nz, ny, nx, lo, hi)
    z = levels(Geom((nz, ny, nx)))
    top = {t: cpo.echo_top(g, z, t, lo, hi, linear) for t in THRESHOLDS}
    base = {t: cpo.echo_base(g, z, t, lo, hi, linear) for t in THRESHOLDS}
    return top, base, cpo.vil(g, z, 56.0, lo, hi)


def check_against_oracle(rg, grid_in, nz, ny, nx, lo, hi, kw, label):
    geom = Geom((nz, ny, nx))
    z32 = set(np.float32(levels(geom)).view(np.int32).tolist())
    for interpolation in ("linear", "nearest"):
        top, base, vil = want_planes(nz, ny, nx, lo, hi, interpolation == "linear")
        got = rg.column_profile(grid_in, geom, echo_top=THRESHOLDS, echo_base=THRESHOLDS, vil=True,
                                interpolation=interpolation, **kw)
        assert list(got) == ["echo_top", "echo_base", "vil"] and list(got["echo_top"]) == list(THRESHOLDS)
        for t in THRESHOLDS:
            assert_bits(got["echo_top"][t], top[t], (label, interpolation, "top", t))
            assert_bits(got["echo_base"][t], base[t], (label, interpolation, "base", t))
            if interpolation == "nearest":
                for plane in (host(got["echo_top"][t]), host(got["echo_base"][t])):
                    vals = plane[~np.isnan(plane)]
                    assert set(vals.view(np.int32).tolist()) <= z32, (label, t)
        assert_vil(got["vil"], vil, (label, interpolation))


# ---- 1. the kernel against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("nz", NZS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_planes_match_the_restatement(env, shape, nz):
    torch, rg = env["torch"], env["rg"]
    ny, nx = SHAPES[shape]
    for lo, hi, kw in windows(nz):
        g = grid_for(nz, ny, nx, lo, hi)
        t = torch.from_numpy(g.copy()).to(env["dev"])
        assert t.data_ptr() % 16 == 0
        check_against_oracle(rg, t, nz, ny, nx, lo, hi, kw, (shape, nz, lo, hi, tuple(kw)))
    # NumPy in -> NumPy out: the same planes
    lo, hi, kw = windows(nz)[-1]
    g = grid_for(nz, ny, nx, lo, hi)
    top, base, vil = want_planes(nz, ny, nx, lo, hi, True)
    geom = Geom((nz, ny, nx))
    got = rg.echo_top(g, geom, 30.0, **kw)
    assert isinstance(got, np.ndarray)
    assert_bits(got, top[30.0], (shape, nz, "numpy top"))
    assert_bits(rg.echo_base(g, geom, **kw), base[18.0], (shape, nz, "numpy base"))
    assert_vil(rg.vertically_integrated_liquid(g, geom, **kw), vil, (shape, nz, "numpy vil"))


@pytest.mark.parametrize("nz", NZS)
def test_unaligned_grid_pointer(env, nz):
    """A (3, 5) grid that starts one float into a device buffer: n_xy % 4 != 0 and the pointer is not 16-byte aligned."""
    torch, rg = env["torch"], env["rg"]
    ny, nx = SHAPES["scalar"]
    for lo, hi, kw in windows(nz):
        g = grid_for(nz, ny, nx, lo, hi)
        big = torch.full((nz * ny * nx + 1,), 99.0, dtype=torch.float32, device=env["dev"])
        big[1:] = torch.from_numpy(g.copy()).reshape(-1).to(env["dev"])
        view = big[1:].view(nz, ny, nx)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        check_against_oracle(rg, view, nz, ny, nx, lo, hi, kw, ("unaligned grid", nz, lo, hi))


@pytest.mark.parametrize("nz", NZS)
@pytest.mark.parametrize("ny, nx", [(2, 6), (2, 8)])
def test_unaligned_output_planes_through_the_c_abi(env, nz, ny, nx):
    """(2, 6): n_xy % 4 == 0 and an aligned grid, but the output planes are slices of a larger buffer at an offset of one
    float -- the one-column path; the floats around the planes stay untouched.  (2, 8) is the same with room for every
    constructed column (the infinite neighbours and the louder echo just outside the window are the last two)."""
    torch, native = env["torch"], env["native"]
    lib = native.load_library()
    assert len(constructed_columns(nz, 0, nz - 1)) <= 2 * 8
    n_xy = ny * nx
    nt = len(THRESHOLDS)
    geom = Geom((nz, ny, nx))
    zl = torch.from_numpy(levels(geom)).to(env["dev"])
    thr = (ctypes.c_double * nt)(*THRESHOLDS)
    for lo, hi, _ in windows(nz):
        g = torch.from_numpy(grid_for(nz, ny, nx, lo, hi).copy()).to(env["dev"])
        top, base, vil = want_planes(nz, ny, nx, lo, hi, True)
        bufs = [torch.full((n + 2,), -7.0, dtype=torch.float32, device=env["dev"]) for n in (nt * n_xy, nt * n_xy, n_xy)]
        outs = [b[1:-1] for b in bufs]
        assert g.data_ptr() % 16 == 0 and all(o.data_ptr() % 16 == 4 for o in outs)
        status = lib.rg_column_profile_f32(native.ptr(g), nz, n_xy, lo, hi, native.ptr(zl), thr, nt, 1, native.ptr(outs[0]),
                                           native.ptr(outs[1]), 56.0, native.ptr(outs[2]), native.stream_ptr())
        native.check(status, "rg_column_profile_f32")
        torch.cuda.synchronize()
        for i, t in enumerate(THRESHOLDS):
            assert_bits(outs[0][i * n_xy:(i + 1) * n_xy].view(ny, nx), top[t], ("abi top", nz, lo, hi, t))
            assert_bits(outs[1][i * n_xy:(i + 1) * n_xy].view(ny, nx), base[t], ("abi base", nz, lo, hi, t))
        assert_vil(outs[2].view(ny, nx), vil, ("abi vil", nz, lo, hi))
        for b in bufs:
            assert float(b[0]) == -7.0 and float(b[-1]) == -7.0


# ---- 2. independence ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["scalar", "vector"])
def test_thresholds_are_independent_and_the_named_functions_agree(env, shape):
    torch, rg = env["torch"], env["rg"]
    nz = 7
    ny, nx = SHAPES[shape]
    lo, hi, kw = windows(nz)[2]
    geom = Geom((nz, ny, nx))
    g = torch.from_numpy(grid_for(nz, ny, nx, lo, hi).copy()).to(env["dev"])
    for interpolation in ("linear", "nearest"):
        both = rg.column_profile(g, geom, echo_top=THRESHOLDS, echo_base=THRESHOLDS, vil=True, max_dbz=50.0,
                                 interpolation=interpolation, **kw)
        for t in THRESHOLDS:
            alone = rg.column_profile(g, geom, echo_top=(t,), interpolation=interpolation, **kw)
            assert list(alone) == ["echo_top"]
            assert torch.equal(alone["echo_top"][t].view(torch.int32), both["echo_top"][t].view(torch.int32))
            assert torch.equal(rg.echo_top(g, geom, t, interpolation, **kw).view(torch.int32),
                               both["echo_top"][t].view(torch.int32))
            assert torch.equal(rg.echo_base(g, geom, t, interpolation, **kw).view(torch.int32),
                               both["echo_base"][t].view(torch.int32))
        assert torch.equal(rg.vertically_integrated_liquid(g, geom, 50.0, **kw).view(torch.int32),
                           both["vil"].view(torch.int32))
    # more than four distinct thresholds, different ones for top and base: further launches, the same planes
    many = (18.0, 30.0, 45.0, -3.5, 10.0, 22.5)
    got = rg.column_profile(g, geom, echo_top=many, echo_base=(22.5, 18.0), **kw)
    assert list(got["echo_top"]) == list(many) and list(got["echo_base"]) == [22.5, 18.0]
    for t in many:
        assert torch.equal(got["echo_top"][t].view(torch.int32), rg.echo_top(g, geom, t, **kw).view(torch.int32))
    for t in (22.5, 18.0):
        assert torch.equal(got["echo_base"][t].view(torch.int32), rg.echo_base(g, geom, t, **kw).view(torch.int32))


def test_threshold_between_two_float32_values(env):
    """The comparison is ``(double)g >= T``: a threshold a hair above or below a float32 value decides as float64 does."""
    torch, rg = env["torch"], env["rg"]
    nz = 7
    geom = Geom((nz, 1, 4))
    z = levels(geom)
    v = np.float32(18.1)                                                      # not a float64 integer multiple of anything handy
    g = np.full((nz, 1, 4), 5.0, dtype=np.float32)
    g[3, 0, :] = v
    g[2, 0, 1] = np.nextafter(v, np.float32(0.0))
    g[4, 0, 2] = np.nextafter(v, np.float32(100.0))
    t = torch.from_numpy(g).to(env["dev"])
    for thr in (float(v), float(np.nextafter(np.float64(v), 100.0)), float(np.nextafter(np.float64(v), 0.0)),
                float(v) + 1e-9, float(v) - 1e-9, 18.1, 1e300, -1e300, 3.5e38, -3.5e38):
        got = rg.column_profile(t, geom, echo_top=(thr,), echo_base=(thr,))
        assert_bits(got["echo_top"][thr], cpo.echo_top(g, z, thr), ("between", thr, "top"))
        assert_bits(got["echo_base"][thr], cpo.echo_base(g, z, thr), ("between", thr, "base"))
    # not vacuous: a hair above the value nothing reaches the threshold, a hair below the level does
    assert np.isnan(cpo.echo_top(g, z, float(v) + 1e-9)[0, 0]) and np.isfinite(cpo.echo_top(g, z, float(v) - 1e-9)[0, 0])


def test_vector_and_one_column_paths_give_the_same_bits(env):
    """A (3, 5) grid padded to (3, 8): the shared columns come out the same on the vector path."""
    torch, rg = env["torch"], env["rg"]
    for nz in (7, 40):
        lo, hi, kw = windows(nz)[2]
        g = grid_for(nz, 3, 5, lo, hi)
        wide = np.full((nz, 3, 8), 33.0, dtype=np.float32)
        wide[:, :, :5] = g
        spec = dict(echo_top=THRESHOLDS, echo_base=THRESHOLDS, vil=True, **kw)
        narrow = rg.column_profile(torch.from_numpy(g.copy()).to(env["dev"]), Geom((nz, 3, 5)), **spec)
        padded = rg.column_profile(torch.from_numpy(wide).to(env["dev"]), Geom((nz, 3, 8)), **spec)
        for t in THRESHOLDS:
            for key in ("echo_top", "echo_base"):
                assert torch.equal(narrow[key][t].view(torch.int32), padded[key][t][:, :5].contiguous().view(torch.int32))
        assert torch.equal(narrow["vil"].view(torch.int32), padded["vil"][:, :5].contiguous().view(torch.int32))


def test_section_shaped_grid(env):
    """The (nz, 1, n_points) stack of the section entry points works unchanged."""
    rg, torch = env["rg"], env["torch"]
    nz, n = 7, 15
    g = grid_for(nz, 3, 5, 0, nz - 1).reshape(nz, 1, n)
    z = levels(Geom((nz, 1, n)))
    got = rg.echo_top(torch.from_numpy(g.copy()).to(env["dev"]), Geom((nz, 1, n)), 30.0)
    assert_bits(got, cpo.echo_top(g, z, 30.0), "section")


# ---- 3. routes ---------------------------------------------------------------------------------------------------------------
PROFILE = dict(echo_top=(18.0, 30.0), echo_base=(18.0,), vil=True)


def assert_record(torch, rg, rec, rec_plain, grid, geom, label, **window):
    """``rec`` holds what column_profile gives on ``grid``, and otherwise the planes of the plain request, bit for bit."""
    want = rg.column_profile(grid, geom, **PROFILE, **window)
    assert set(rec) == set(rec_plain) | {"echo_top", "echo_base", "vil"} and not set(rec_plain) & {"echo_top", "echo_base", "vil"}
    for key in ("echo_top", "echo_base"):
        assert list(rec[key]) == list(want[key]), label
        for t in want[key]:
            assert torch.equal(rec[key][t].view(torch.int32), want[key][t].view(torch.int32)), (label, key, t)
    assert torch.equal(rec["vil"].view(torch.int32), want["vil"].view(torch.int32)), label
    for key, plane in rec_plain.items():
        if isinstance(plane, dict):
            assert list(plane) == list(rec[key])
            for a, p in plane.items():
                assert torch.equal(p.view(torch.int32), rec[key][a].view(torch.int32)), (label, key, a)
        else:
            assert plane.dtype == rec[key].dtype and torch.equal(plane.view(torch.int32), rec[key].view(torch.int32)), (label, key)
    return int(torch.isfinite(rec["echo_top"][18.0]).sum()), int(torch.isfinite(rec["vil"]).sum())


@functools.lru_cache(maxsize=None)
def small_volumes():
    from radar_processor_amd import synthetic
    return [synthetic.make_volume(n_elev=4, n_az=90, n_gates=100, seed=20 + b, fields=("DBZH", "ZDR")) for b in range(3)]


SMALL_SHAPE, SMALL_LIMITS = (5, 9, 13), ((0.0, 6000.0), (-50e3, 50e3), (-60e3, 60e3))


def test_route_grid_products_device_on_a_csr_geometry(env, tmp_path):
    torch, rg, dev = env["torch"], env["rg"], env["dev"]
    vol = small_volumes()[0]
    geom = rg.compute_grid_geometry(vol.gate_x, vol.gate_y, vol.gate_z, SMALL_SHAPE, SMALL_LIMITS, str(tmp_path))
    fields = [torch.from_numpy(np.ma.getdata(vol.fields[k]).astype(np.float32)).to(dev) for k in ("DBZH", "ZDR")]
    masks = [torch.from_numpy(np.ma.getmaskarray(vol.fields[k]).astype(np.uint8)).to(dev) for k in ("DBZH", "ZDR")]
    grids = rg.grid_fields_device(geom, fields, masks)
    window = dict(z_min_idx=1, z_max_idx=3)
    plain = rg.PlaneProducts(cappi=(2000.0,), colmean=True, **window)
    spec = rg.PlaneProducts(cappi=(2000.0,), colmean=True, **window, **PROFILE)
    hits = (0, 0)
    for fused in (None, False):
        recs = rg.grid_products_device(geom, fields, masks, products=spec, fused=fused)
        recs_plain = rg.grid_products_device(geom, fields, masks, products=plain, fused=fused)
        for k in range(2):
            hits = assert_record(torch, rg, recs[k], recs_plain[k], grids[k], geom, ("csr", fused, k), **window)
        assert list(recs[0])[-3:] == ["echo_top", "echo_base", "vil"]
    with pytest.raises(ValueError, match="fused=True"):
        rg.grid_products_device(geom, fields, masks, products=spec, fused=True)
    recs = rg.grid_products_device(geom, fields[:1], masks[:1], products=rg.PlaneProducts(**PROFILE))
    first = assert_record(torch, rg, recs[0], rg.grid_products_device(geom, fields[:1], masks[:1])[0], grids[0], geom, "csr full")
    assert first[0] > 0 and first[1] > 0 and hits[1] > 0                      # the scene reaches 18 dBZ: not vacuous


@pytest.mark.parametrize("combine", ["mean", "max"])
def test_route_two_radar_mosaic_search(env, combine):
    torch, rg, dev = env["torch"], env["rg"], env["dev"]
    scene = mosaic_scenes.scene16()
    sel = [1, 4]
    assert [scene.kinds[r] for r in sel] == ["live", "live"]
    ms = rg.MosaicSearch(scene.radars(sel), scene.shape, scene.limits, min_radius=mosaic_scenes.MIN_RADIUS,
                         toa=mosaic_scenes.TOA)
    fields = [[torch.from_numpy(np.ma.getdata(scene.vols[r].fields["DBZH"]).astype(np.float32)).to(dev)] for r in sel]
    masks = [[torch.from_numpy(np.ma.getmaskarray(scene.vols[r].fields["DBZH"]).astype(np.uint8)).to(dev)] for r in sel]
    grids = rg.mosaic_fields_device(ms, fields, masks, combine=combine)
    recs = rg.mosaic_fields_device(ms, fields, masks, combine=combine, products=rg.PlaneProducts(**PROFILE))
    plain = rg.mosaic_fields_device(ms, fields, masks, combine=combine, products=rg.PlaneProducts())
    hits = assert_record(torch, rg, recs[0], plain[0], grids[0], ms, ("mosaic", combine))
    assert hits[1] > 0


def test_route_volume_batch_on_a_csr_geometry_and_a_roi_search(env, tmp_path):
    torch, rg, dev = env["torch"], env["rg"], env["dev"]
    from radar_processor_amd import batch
    vols = small_volumes()
    geom = rg.compute_grid_geometry(vols[0].gate_x, vols[0].gate_y, vols[0].gate_z, SMALL_SHAPE, SMALL_LIMITS, str(tmp_path))
    search = rg.RoiSearch(vols[0].gate_x, vols[0].gate_y, vols[0].gate_z, SMALL_SHAPE, SMALL_LIMITS, device=dev)
    volumes = [{k: (np.ma.getdata(v.fields[k]), np.ma.getmaskarray(v.fields[k])) for k in ("DBZH", "ZDR")} for v in vols]
    window = dict(z_min_alt=1000.0, z_max_alt=5000.0)
    for geometry in (geom, search):
        vb = batch.VolumeBatch(geometry, ["DBZH", "ZDR"], device=dev)
        grids = vb.grid_shard(volumes)
        recs = vb.grid_shard(volumes, products=rg.PlaneProducts(**window, **PROFILE))
        plain = vb.grid_shard(volumes, products=rg.PlaneProducts(**window))
        assert sorted(recs) == [0, 1, 2]
        for b in range(3):
            for i in range(2):
                assert_record(torch, rg, recs[b][i], plain[b][i], grids[b][i], geometry, ("batch", vb.fused, b, i), **window)
