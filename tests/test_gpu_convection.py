"""Convective / stratiform classification on the GPU (csrc/rg_convection.hip, radar_processor_amd/convection.py) against the
NumPy restatement of tests/convection_oracle.py on the scenes of tests/convection_scenes.py, through the raw C ABI between
canaries and through the public functions.

The device may differ from NumPy in two places only: one unit of q at a rounding tie of exp10, and one float32 step of the
background's log10.  So the stages are chained: q within one unit; S and N EQUAL to the oracle fed the device's q; the
background within one float32 step of the oracle's value from those S and N; the centres EQUAL to the oracle fed the device's
background; the area EQUAL to the oracle fed the device's centres.  On the main scenes, where no decision is fragile, the
whole chain equals the oracle end to end."""
import ctypes
import types

import numpy as np
import pytest

import convection_oracle as co
import convection_scenes as sc

pytestmark = pytest.mark.gpu
CANARY = 64                       # elements before and after every output
_PATTERN = {"int32": -1234567, "int64": -1234567890123, "float32": -12345.5, "uint8": 0xA5}
RG_EINVAL, RG_EALIGN, RG_EWORKSPACE = -1, -2, -4


@pytest.fixture(scope="module")
def env():
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native
    lib = rg.load_library()
    return dict(torch=torch, rg=rg, native=_native, lib=lib, dev=torch.device("cuda", 0))


def _guarded(env, shape, dtype):
    """``(buffer, view)``: ``view`` of ``shape`` inside a buffer with CANARY pattern elements on either side."""
    torch = env["torch"]
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * CANARY,), _PATTERN[dtype], dtype=getattr(torch, dtype), device=env["dev"])
    return buf, buf[CANARY:CANARY + n].view(shape)


def _intact(buf, n):
    host = buf.cpu().numpy()
    edge = np.concatenate([host[:CANARY], host[CANARY + n:]])
    return bool((edge == edge.dtype.type(_PATTERN[str(edge.dtype)])).all())


def _untouched(buf):
    host = buf.cpu().numpy()
    return bool((host == host.dtype.type(_PATTERN[str(host.dtype)])).all())


def _dev(env, a):
    return None if a is None else env["torch"].from_numpy(np.array(a)).to(env["dev"])     # a copy: the scenes are read-only


def _c(ctype, values):
    return (ctype * max(len(values), 1))(*values)


def _area_tables(footprints):
    rows = (ctypes.c_int32 * (len(footprints) * 128))()
    for k, hw in enumerate(footprints):
        rows[k * 128:k * 128 + len(hw)] = hw
    return rows, _c(ctypes.c_int32, [len(hw) - 1 for hw in footprints])


def _raw(env, s):
    """The staged entry points between canaries; ``run()`` returns every output as an array and may be called again into
    the same buffers."""
    torch, nat, lib = env["torch"], env["native"], env["lib"]
    shape = n, h, w = s.dbz.shape
    K = len(s.footprints)
    f, m = _dev(env, s.dbz), _dev(env, s.mask)
    table_bytes, ws_bytes = int(lib.rg_echo_table_bytes(n, h, w)), int(lib.rg_convective_area_workspace_bytes(n, h, w, K))
    assert table_bytes >= n * h * w * 12 and ws_bytes >= n * h * w * K * 4
    bufs = dict(table=_guarded(env, (table_bytes,), "uint8"), workspace=_guarded(env, (ws_bytes,), "uint8"),
                q=_guarded(env, shape, "int64"), flag=_guarded(env, shape, "int32"), S=_guarded(env, shape, "int64"),
                N=_guarded(env, shape, "int32"), bkg=_guarded(env, shape, "float32"), centres=_guarded(env, shape, "uint8"),
                classes=_guarded(env, shape, "uint8"))
    hw0, hw = _c(ctypes.c_int32, [0]), _c(ctypes.c_int32, s.hw)
    rows, ry = _area_tables(s.footprints)
    edges = _c(ctypes.c_double, s.edges)

    def run():
        v = {k: b[1] for k, b in bufs.items()}
        stream = nat.stream_ptr()
        with torch.cuda.device(env["dev"]):
            assert lib.rg_echo_table_f32(nat.ptr(f), nat.ptr(m), n, h, w, s.min_dbz, nat.ptr(v["table"]), table_bytes, stream) == 0
            assert lib.rg_disk_background(nat.ptr(v["table"]), n, h, w, hw0, 0, nat.ptr(v["q"]), nat.ptr(v["flag"]), None, stream) == 0
            assert lib.rg_disk_background(nat.ptr(v["table"]), n, h, w, hw, len(s.hw) - 1, nat.ptr(v["S"]), nat.ptr(v["N"]),
                                          nat.ptr(v["bkg"]), stream) == 0
            assert lib.rg_convective_centres_f32(nat.ptr(f), nat.ptr(m), nat.ptr(v["bkg"]), n, h, w, s.min_dbz, s.intense, s.peak[0],
                                                 s.peak[1], edges, len(s.edges) + 1, nat.ptr(v["centres"]), stream) == 0
            assert lib.rg_convective_area_u8(nat.ptr(v["centres"]), nat.ptr(f), nat.ptr(m), n, h, w, s.min_dbz, K, rows, ry,
                                             nat.ptr(v["workspace"]), ws_bytes, nat.ptr(v["classes"]), stream) == 0
        torch.cuda.synchronize()
        for key, (buf, view) in bufs.items():
            assert _intact(buf, view.numel()), key
        return {k: view.cpu().numpy() for k, view in v.items() if k not in ("table", "workspace")}

    return run, (f, m)


def _within_one_step(got, want):
    """float32 arrays: NaN in the same places and every other value equal to ``want`` or to one of its two neighbours."""
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    g, t = got[~nan], want[~nan]
    return bool(((g == t) | (g == np.nextafter(t, np.float32(np.inf))) | (g == np.nextafter(t, np.float32(-np.inf)))).all())


# ---- the raw C ABI against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.SCENES)
def test_every_stage_equals_the_restatement_fed_the_stage_before(env, name):
    s, want = sc.scene(name), sc.expected(name)
    run, (f, m) = _raw(env, s)
    got = run()
    # q through the radius-0 call: within one unit of NumPy's, the echo flags equal
    assert int(np.abs(got["q"] - want.q).max()) <= 1, (name, int(np.abs(got["q"] - want.q).max()))
    assert np.array_equal(got["flag"], want.echo.astype(np.int32)) and np.array_equal(got["q"] > 0, want.echo)
    # S and N: equal to the oracle fed the device's q
    S, N, _ = co.background(s.dbz, s.hw, s.mask, s.min_dbz, q=got["q"])
    assert np.array_equal(got["S"], S), f"{name}: {int((got['S'] != S).sum())} sums differ"
    assert np.array_equal(got["N"], N) and np.array_equal(N, want.N)
    # the background: within one float32 step of the oracle's value from those S and N
    assert _within_one_step(got["bkg"], co.background_from_sums(got["S"], got["N"])), name
    # centres and area: equal to the oracle fed the device's stage before
    assert np.array_equal(got["centres"], co.centres(s.dbz, got["bkg"], s.edges, s.mask, s.min_dbz, s.intense, s.peak)), name
    assert np.array_equal(got["classes"], co.area(got["centres"], s.dbz, s.footprints, s.mask, s.min_dbz)), name
    # inputs byte-unchanged
    assert f.cpu().numpy().tobytes() == s.dbz.tobytes() and (m is None or m.cpu().numpy().tobytes() == s.mask.tobytes())
    # a second pass into the same buffers: the same bytes
    again = run()
    for key in got:
        assert again[key].tobytes() == got[key].tobytes(), (name, key)


def test_big_sums_are_exact_beyond_float64s_integers(env):
    s, want = sc.scene("big_sums"), sc.expected("big_sums")
    run, _ = _raw(env, s)
    got = run()
    assert np.array_equal(got["S"], want.S) and int(got["S"].max()) == 51101 * 65536 * 10 ** 8 > 2 ** 53
    assert (got["bkg"] == np.float32(80.0)).all() and (got["classes"] == 2).all()


def test_each_output_of_the_background_alone(env):
    """Any one of the three outputs may be asked for alone and holds the bits of the full call."""
    torch, nat, lib = env["torch"], env["native"], env["lib"]
    s = sc.scene("seam_257")
    n, h, w = s.dbz.shape
    full = _raw(env, s)[0]()
    f, m = _dev(env, s.dbz), _dev(env, s.mask)
    table = torch.empty(int(lib.rg_echo_table_bytes(n, h, w)), dtype=torch.uint8, device=env["dev"])
    assert lib.rg_echo_table_f32(nat.ptr(f), nat.ptr(m), n, h, w, s.min_dbz, nat.ptr(table), table.numel(), nat.stream_ptr()) == 0
    for key, dtype, slot in (("S", "int64", 0), ("N", "int32", 1), ("bkg", "float32", 2)):
        buf, view = _guarded(env, s.dbz.shape, dtype)
        outs = [None, None, None]
        outs[slot] = nat.ptr(view)
        assert lib.rg_disk_background(nat.ptr(table), n, h, w, _c(ctypes.c_int32, s.hw), len(s.hw) - 1, *outs, nat.stream_ptr()) == 0
        torch.cuda.synchronize()
        assert _intact(buf, view.numel()) and view.cpu().numpy().tobytes() == full[key].tobytes(), key


def test_empty_planes_return_ok_without_touching_anything(env):
    nat, lib = env["native"], env["lib"]
    hw = _c(ctypes.c_int32, [1, 1])
    for h, w in ((0, 9), (9, 0), (0, 0)):
        assert lib.rg_echo_table_bytes(2, h, w) == 0 and lib.rg_convective_area_workspace_bytes(2, h, w, 3) == 0
        table, out = _guarded(env, (64,), "uint8"), _guarded(env, (64,), "float32")
        cls, ws = _guarded(env, (64,), "uint8"), _guarded(env, (64,), "uint8")
        f = env["torch"].zeros(64, dtype=env["torch"].float32, device=env["dev"])
        assert lib.rg_echo_table_f32(nat.ptr(f), None, 2, h, w, 5.0, nat.ptr(table[1]), 0, nat.stream_ptr()) == 0
        assert lib.rg_disk_background(nat.ptr(table[1]), 2, h, w, hw, 1, None, None, nat.ptr(out[1]), nat.stream_ptr()) == 0
        assert lib.rg_convective_centres_f32(nat.ptr(f), None, nat.ptr(out[1]), 2, h, w, 5.0, 40.0, 10.0, 180.0, None, 1,
                                             nat.ptr(cls[1]), nat.stream_ptr()) == 0
        rows, ry = _area_tables(((1, 1),))
        assert lib.rg_convective_area_u8(nat.ptr(cls[1]), nat.ptr(f), None, 2, h, w, 5.0, 1, rows, ry, nat.ptr(ws[1]), 0,
                                         nat.ptr(table[1]), nat.stream_ptr()) == 0
        env["torch"].cuda.synchronize()
        assert all(_untouched(b[0]) for b in (table, out, cls, ws)), (h, w)


def test_every_refused_call_leaves_the_canaries_untouched(env):
    torch, nat, lib = env["torch"], env["native"], env["lib"]
    n, h, w, K = 1, 6, 10, 2
    f = torch.full((n, h, w), 30.0, dtype=torch.float32, device=env["dev"])
    m = torch.zeros((n, h, w), dtype=torch.uint8, device=env["dev"])
    need, ws_need = int(lib.rg_echo_table_bytes(n, h, w)), int(lib.rg_convective_area_workspace_bytes(n, h, w, K))
    table, ws = _guarded(env, (need,), "uint8"), _guarded(env, (ws_need,), "uint8")
    S, N, bkg = _guarded(env, (n, h, w), "int64"), _guarded(env, (n, h, w), "int32"), _guarded(env, (n, h, w), "float32")
    cen, cls = _guarded(env, (n, h, w), "uint8"), _guarded(env, (n, h, w), "uint8")
    P = nat.ptr
    stream = nat.stream_ptr()
    inf, nan = float("inf"), float("nan")
    hw, bad_hw, neg_hw = _c(ctypes.c_int32, [2, 1]), _c(ctypes.c_int32, [2, 128]), _c(ctypes.c_int32, [-1, 1])
    edges, down, nf = _c(ctypes.c_double, [25.0]), _c(ctypes.c_double, [30.0, 25.0]), _c(ctypes.c_double, [nan])
    rows, ry = _area_tables(((1, 1), (2, 2, 1)))
    bad_rows, _ = _area_tables(((1, 200), (2, 2, 1)))
    bad_ry = _c(ctypes.c_int32, [1, 128])

    def table_call(dbz=P(f), mask=P(m), n_=n, h_=h, w_=w, min_dbz=5.0, t=P(table[1]), b=need):
        return lib.rg_echo_table_f32(dbz, mask, n_, h_, w_, min_dbz, t, b, stream)

    def disk_call(t=P(table[1]), n_=n, h_=h, w_=w, hw_=hw, ry_=1, s=P(S[1]), c=P(N[1]), b=P(bkg[1])):
        return lib.rg_disk_background(t, n_, h_, w_, hw_, ry_, s, c, b, stream)

    def centre_call(dbz=P(f), b=P(bkg[1]), n_=n, h_=h, w_=w, min_dbz=5.0, intense=40.0, pa=10.0, pb=180.0, e=edges, k=2, out=P(cen[1])):
        return lib.rg_convective_centres_f32(dbz, P(m), b, n_, h_, w_, min_dbz, intense, pa, pb, e, k, out, stream)

    def area_call(c=P(cen[1]), dbz=P(f), n_=n, h_=h, w_=w, min_dbz=5.0, k=K, r=rows, y=ry, wsp=P(ws[1]), b=ws_need, out=P(cls[1])):
        return lib.rg_convective_area_u8(c, dbz, P(m), n_, h_, w_, min_dbz, k, r, y, wsp, b, out, stream)

    refused = [
        (table_call(dbz=None), RG_EINVAL), (table_call(t=None), RG_EINVAL), (table_call(n_=0), RG_EINVAL),
        (table_call(n_=65536), RG_EINVAL), (table_call(h_=-1), RG_EINVAL), (table_call(h_=65536, w_=32768), RG_EINVAL),
        (table_call(min_dbz=nan), RG_EINVAL), (table_call(min_dbz=inf), RG_EINVAL), (table_call(b=need - 1), RG_EWORKSPACE),
        (table_call(t=P(table[1]) + 4), RG_EALIGN), (table_call(dbz=P(table[1])), RG_EINVAL),
        (table_call(mask=P(table[1]) + 16), RG_EINVAL),
        (disk_call(t=None), RG_EINVAL), (disk_call(hw_=None), RG_EINVAL), (disk_call(s=None, c=None, b=None), RG_EINVAL),
        (disk_call(n_=0), RG_EINVAL), (disk_call(w_=-3), RG_EINVAL), (disk_call(ry_=-1), RG_EINVAL), (disk_call(ry_=128), RG_EINVAL),
        (disk_call(hw_=bad_hw), RG_EINVAL), (disk_call(hw_=neg_hw), RG_EINVAL), (disk_call(t=P(table[1]) + 8), RG_EALIGN),
        (disk_call(s=P(table[1])), RG_EINVAL), (disk_call(b=P(S[1])), RG_EINVAL), (disk_call(c=P(bkg[1]) + 4), RG_EINVAL),
        (centre_call(dbz=None), RG_EINVAL), (centre_call(b=None), RG_EINVAL), (centre_call(out=None), RG_EINVAL),
        (centre_call(n_=0), RG_EINVAL), (centre_call(h_=-1), RG_EINVAL), (centre_call(k=0), RG_EINVAL), (centre_call(k=9), RG_EINVAL),
        (centre_call(e=None), RG_EINVAL), (centre_call(e=down, k=3), RG_EINVAL), (centre_call(e=nf), RG_EINVAL),
        (centre_call(min_dbz=nan), RG_EINVAL), (centre_call(intense=inf), RG_EINVAL), (centre_call(pa=nan), RG_EINVAL),
        (centre_call(pb=inf), RG_EINVAL), (centre_call(pb=0.0), RG_EINVAL), (centre_call(pb=-180.0), RG_EINVAL),
        (centre_call(out=P(f)), RG_EINVAL), (centre_call(out=P(bkg[1]) + 8), RG_EINVAL), (centre_call(out=P(m)), RG_EINVAL),
        (area_call(c=None), RG_EINVAL), (area_call(dbz=None), RG_EINVAL), (area_call(r=None), RG_EINVAL), (area_call(y=None), RG_EINVAL),
        (area_call(out=None), RG_EINVAL), (area_call(wsp=None), RG_EINVAL), (area_call(n_=0), RG_EINVAL), (area_call(w_=-1), RG_EINVAL),
        (area_call(k=0), RG_EINVAL), (area_call(k=9), RG_EINVAL), (area_call(min_dbz=-inf), RG_EINVAL),
        (area_call(r=bad_rows), RG_EINVAL), (area_call(y=bad_ry), RG_EINVAL), (area_call(b=ws_need - 1), RG_EWORKSPACE),
        (area_call(wsp=P(ws[1]) + 1), RG_EINVAL), (area_call(out=P(cen[1])), RG_EINVAL), (area_call(out=P(f) + 8), RG_EINVAL),
        (area_call(out=P(m)), RG_EINVAL), (area_call(wsp=P(f)), RG_EINVAL), (area_call(out=P(ws[1]) + 4), RG_EINVAL),
    ]
    assert lib.rg_echo_table_bytes(0, h, w) == RG_EINVAL and lib.rg_echo_table_bytes(1, -1, w) == RG_EINVAL
    assert lib.rg_echo_table_bytes(1, 65536, 32768) == RG_EINVAL and lib.rg_convective_area_workspace_bytes(1, h, w, 9) == RG_EINVAL
    assert lib.rg_convective_area_workspace_bytes(1, h, w, 0) == RG_EINVAL
    torch.cuda.synchronize()
    for index, (status, want) in enumerate(refused):
        assert status == want, (index, status, want, lib.rg_last_error().decode())
    for name, (buf, _) in dict(table=table, ws=ws, S=S, N=N, bkg=bkg, cen=cen, cls=cls).items():
        assert _untouched(buf), name
    assert (f.cpu().numpy() == 30.0).all() and not m.cpu().numpy().any()
    # and the same arguments, unspoilt, are accepted
    assert table_call() == 0 and disk_call() == 0 and centre_call() == 0 and area_call() == 0
    torch.cuda.synchronize()
    assert (cls[1].cpu().numpy() == 1).all() and (N[1].cpu().numpy()[0, 3, 5] == 5 + 3 + 3)


# ---- the public functions ----------------------------------------------------------------------------------------------------
def _geometry(h, w, nz=1):
    """Anything with ``grid_shape`` and ``grid_limits``: steps of DY x DX metres, levels 2000 m apart from 2000 m."""
    return types.SimpleNamespace(grid_shape=(nz, h, w),
                                 grid_limits=((2000.0, 2000.0 + 1000.0 * (nz - 1)), (-1000.0, -1000.0 + sc.DY * (h - 1)),
                                              (500.0, 500.0 + sc.DX * (w - 1))))


@pytest.mark.parametrize("name", sc.MAIN)
def test_main_scenes_equal_the_oracle_end_to_end(env, name):
    rg = env["rg"]
    s, want = sc.scene(name), sc.expected(name)
    staged = _raw(env, s)[0]()
    parts = rg.convective_stratiform_device(_dev(env, s.dbz), dx=sc.DX, dy=sc.DY, mask=_dev(env, s.mask), return_parts=True)
    assert isinstance(parts, rg.ConvectiveStratiform) and parts.classes.dtype == env["torch"].uint8
    # the composite call returns the bits of the staged calls
    assert parts.classes.cpu().numpy().tobytes() == staged["classes"].tobytes()
    assert parts.background.cpu().numpy().tobytes() == staged["bkg"].tobytes()
    assert parts.centres.cpu().numpy().tobytes() == staged["centres"].tobytes()
    # and equals the oracle end to end, no pixel left out
    assert np.array_equal(parts.centres.cpu().numpy(), want.centres), int((parts.centres.cpu().numpy() != want.centres).sum())
    assert np.array_equal(parts.classes.cpu().numpy(), want.classes), int((parts.classes.cpu().numpy() != want.classes).sum())
    assert _within_one_step(parts.background.cpu().numpy(), want.bkg) or np.abs(parts.background.cpu().numpy() - want.bkg)[want.N > 0].max() < 1e-4
    # arrays in, arrays out; one plane; the spacing from a geometry
    plain = rg.convective_stratiform(s.dbz[0], dx=sc.DX, dy=sc.DY, mask=s.mask[0])
    assert isinstance(plain, np.ndarray) and plain.shape == s.dbz.shape[1:] and np.array_equal(plain, want.classes[0])
    by_geometry = rg.convective_stratiform(s.dbz, geometry=_geometry(*s.dbz.shape[1:]), mask=s.mask, return_parts=True)
    assert all(isinstance(a, np.ndarray) for a in by_geometry) and np.array_equal(by_geometry.classes, want.classes)
    assert by_geometry.background.tobytes() == staged["bkg"].tobytes()
    # the background as a product
    bkg, count = rg.echo_background_device(s.dbz, dx=sc.DX, dy=sc.DY, mask=s.mask, return_counts=True)
    assert bkg.cpu().numpy().tobytes() == staged["bkg"].tobytes() and np.array_equal(count.cpu().numpy(), want.N)
    assert rg.echo_background_device(_dev(env, s.dbz[0]), dx=sc.DX, dy=sc.DY, mask=s.mask[0]).cpu().numpy().tobytes() == staged["bkg"].tobytes()


def test_relations_stacks_and_known_answers_through_the_public_call(env):
    rg = env["rg"]
    s, want = sc.scene("stack"), sc.expected("stack")
    got = rg.convective_stratiform(s.dbz, dx=sc.DX, dy=sc.DY, mask=s.mask, return_parts=True)
    assert np.array_equal(got.centres, co.centres(s.dbz, got.background, s.edges, s.mask))
    assert np.array_equal(got.classes, co.area(got.centres, s.dbz, s.footprints, s.mask)) and not got.classes[1].any()
    assert np.isnan(got.background[1]).all() and np.array_equal(np.isnan(got.background), want.N == 0)
    for p in range(3):                                                      # every plane alone equals its slice
        one = rg.convective_stratiform(s.dbz[p], dx=sc.DX, dy=sc.DY, mask=s.mask[p])
        assert np.array_equal(one, got.classes[p]), p
    # another relation: its edges, radii and peak curve reach the kernels
    edges, radii, peak = (22.0, 33.0), (800.0, 2400.0, 3300.0), (8.0, 150.0)
    other = rg.convective_stratiform(s.dbz, dx=sc.DX, dy=sc.DY, mask=s.mask, min_dbz=7.5, intense=43.0, peak_relation=peak,
                                     area_relation=(edges, radii), background_radius=6000.0, return_parts=True)
    hw, fps = sc.footprint(6000.0), [sc.footprint(r) for r in radii]
    S, N, _ = co.background(s.dbz, hw, s.mask, 7.5)
    assert np.array_equal(np.isnan(other.background), N == 0)
    assert np.array_equal(other.centres, co.centres(s.dbz, other.background, edges, s.mask, 7.5, 43.0, peak))
    assert np.array_equal(other.classes, co.area(other.centres, s.dbz, fps, s.mask, 7.5))
    for preset in ("small", "large"):
        e, r = rg.convection.AREA_RELATIONS[preset]
        part = rg.convective_stratiform(s.dbz[0], dx=sc.DX, dy=sc.DY, area_relation=preset, return_parts=True)
        assert np.array_equal(part.centres, co.centres(s.dbz[0], part.background, e))
        assert np.array_equal(part.classes, co.area(part.centres, s.dbz[0], [sc.footprint(x) for x in r])[0])
    # known answers
    assert (rg.convective_stratiform(sc.uniform(20.0), dx=sc.DX, dy=sc.DY) == 1).all()
    assert (rg.convective_stratiform(sc.uniform(45.0), dx=sc.DX, dy=sc.DY) == 2).all()
    planes, at = sc.spike()
    spiked = rg.convective_stratiform(planes, dx=sc.DX, dy=sc.DY, return_parts=True)
    disk = sc.footprint_mask(rg.disk_footprint(1000.0, sc.DY, sc.DX), planes.shape[1:], at)
    assert spiked.centres.sum() == 1 and spiked.centres[0][at] == 1 and np.array_equal(spiked.classes[0] == 2, disk)


def test_classify_grid_takes_the_cappi_of_the_work_level(env):
    rg = env["rg"]
    s = sc.scene("main_39")
    h, w = s.dbz.shape[1:]
    other, _ = sc.field(12, (h, w))
    grid = np.stack([other, s.dbz[0], other])                               # levels at 2000, 3000, 4000 m
    geometry = _geometry(h, w, nz=3)
    want = sc.expected("main_39")
    got = rg.classify_grid(grid, geometry, mask=s.mask[0])                  # 3000 m: the middle level itself
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want.classes[0])
    # between two levels: the plane the product route gives, classified
    device_grid = _dev(env, grid)
    plane = rg.constant_altitude_ppi(device_grid, geometry, 2400.0)
    blend = rg.classify_grid(device_grid, geometry, altitude=2400.0, area_relation="small", return_parts=True)
    direct = rg.convective_stratiform_device(plane, dx=sc.DX, dy=sc.DY, area_relation="small", return_parts=True)
    for a, b in zip(blend, direct):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert (blend.classes == 2).any() and (blend.classes == 1).any()
    with pytest.raises(ValueError):
        rg.classify_grid(grid, geometry, dx=400.0)


def test_rain_rate_by_class_selects_between_two_rate_planes(env):
    rg = env["rg"]
    s, want = sc.scene("main_35"), sc.expected("main_35")
    classes = _dev(env, want.classes)
    got = rg.rain_rate_by_class_device(_dev(env, s.dbz), classes, mask=_dev(env, s.mask)).cpu().numpy()
    calm = rg.rain_rate_device(s.dbz, a=200.0, b=1.6, mask=s.mask).cpu().numpy()
    heavy = rg.rain_rate_device(s.dbz, a=300.0, b=1.4, mask=s.mask).cpu().numpy()
    assert got.tobytes() == np.where(want.classes == 2, heavy, calm).tobytes()
    assert (calm != heavy)[want.classes == 2].any() and np.isnan(got[s.mask != 0]).all()
    other = rg.rain_rate_by_class_device(s.dbz[0], want.classes[0], stratiform=(250.0, 1.5), convective=(500.0, 1.3), min_dbz=10.0,
                                         max_dbz=50.0).cpu().numpy()
    pair = [rg.rain_rate_device(s.dbz[0], a=a, b=b, min_dbz=10.0, max_dbz=50.0).cpu().numpy() for a, b in ((250.0, 1.5), (500.0, 1.3))]
    assert other.tobytes() == np.where(want.classes[0] == 2, pair[1], pair[0]).tobytes()


def test_the_accumulator_by_class_and_unchanged_without_it(env):
    rg = env["rg"]
    s, want = sc.scene("main_35"), sc.expected("main_35")
    later, _ = sc.field(35, s.dbz.shape[1:])
    later = np.roll(later, 2, axis=1)
    plain = rg.RainAccumulator(motion=None)
    same = rg.RainAccumulator(motion=None, convective_zr=None)
    by_class = rg.RainAccumulator(motion=None, convective_zr=(300.0, 1.4), classify=dict(dx=sc.DX, dy=sc.DY))
    frames = [[acc.update(plane, t, mask=s.mask[0]) for plane, t in ((s.dbz[0], 0.0), (later, 300.0))] for acc in (plain, same, by_class)]
    rate = rg.rain_rate_device(s.dbz[0], mask=s.mask[0]).cpu().numpy()
    for a, b in zip(frames[0], frames[1]):                                  # None classifies nothing: today's bits
        assert a.rate.cpu().numpy().tobytes() == b.rate.cpu().numpy().tobytes()
    assert frames[0][0].rate.cpu().numpy().tobytes() == rate.tobytes()
    assert frames[0][1].interval_mm.cpu().numpy().tobytes() == frames[1][1].interval_mm.cpu().numpy().tobytes()
    expected = rg.rain_rate_by_class_device(s.dbz[0], want.classes[0], mask=s.mask[0]).cpu().numpy()
    assert frames[2][0].rate.cpu().numpy().tobytes() == expected.tobytes() and expected.tobytes() != rate.tobytes()
    depth = rg.accumulate_device(frames[2][0].rate, frames[2][1].rate, None, 300.0 / 3600.0, steps=1).cpu().numpy()
    assert frames[2][1].interval_mm.cpu().numpy().tobytes() == depth.tobytes()
    for bad in (dict(convective_zr=(300.0, 1.4)), dict(classify=dict(dx=400.0)), dict(convective_zr=(0.0, 1.4), classify=dict(dx=400.0)),
                dict(convective_zr=300.0, classify=dict(dx=400.0)), dict(convective_zr=(300.0, 1.4), classify=dict(dx=400.0, radius=3.0)),
                dict(convective_zr=(300.0, 1.4), classify=dict(dx=400.0, area_relation="huge"))):
        with pytest.raises(ValueError):
            rg.RainAccumulator(motion=None, **bad)


def test_value_errors_before_the_device_is_touched(env):
    rg = env["rg"]
    planes = np.zeros((4, 5), np.float32)
    bad_calls = [
        lambda: rg.convective_stratiform_device(planes),                                             # no spacing
        lambda: rg.convective_stratiform_device(planes, dx=400.0, geometry=_geometry(4, 5)),
        lambda: rg.convective_stratiform_device(planes, geometry=_geometry(5, 4)),
        lambda: rg.convective_stratiform_device(planes, dx=0.0),
        lambda: rg.convective_stratiform_device(planes, dx=400.0, dy=float("nan")),
        lambda: rg.convective_stratiform_device(planes.astype(np.float64), dx=400.0),
        lambda: rg.convective_stratiform_device(planes[0], dx=400.0),
        lambda: rg.convective_stratiform_device(planes, dx=400.0, mask=np.zeros((4, 4), np.uint8)),
        lambda: rg.convective_stratiform_device(planes, dx=400.0, min_dbz=float("inf")),
        lambda: rg.convective_stratiform_device(planes, dx=400.0, intense=float("nan")),
        lambda: rg.convective_stratiform_device(planes, dx=400.0, peak_relation="houze"),
        lambda: rg.convective_stratiform_device(planes, dx=400.0, peak_relation=(10.0, 0.0)),
        lambda: rg.convective_stratiform_device(planes, dx=400.0, peak_relation=(10.0,)),
        lambda: rg.convective_stratiform_device(planes, dx=400.0, area_relation="tiny"),
        lambda: rg.convective_stratiform_device(planes, dx=400.0, area_relation=((30.0, 25.0), (1e3, 2e3, 3e3))),
        lambda: rg.convective_stratiform_device(planes, dx=400.0, area_relation=((25.0,), (1e3, 2e3, 3e3))),
        lambda: rg.convective_stratiform_device(planes, dx=400.0, area_relation=((), ())),
        lambda: rg.convective_stratiform_device(planes, dx=400.0, area_relation=(tuple(range(8)), (1e3,) * 9)),
        lambda: rg.convective_stratiform_device(planes, dx=400.0, area_relation=((25.0,), (1e3, -2e3))),
        lambda: rg.convective_stratiform_device(planes, dx=400.0, area_relation=((25.0,), (1e3, 60e3))),   # 150 pixels
        lambda: rg.convective_stratiform_device(planes, dx=40.0),                                    # 11 km: 275 pixels
        lambda: rg.convective_stratiform_device(planes, dx=400.0, background_radius=-1.0),
        lambda: rg.echo_background_device(planes, dx=400.0, radius=60e3),
        lambda: rg.echo_background_device(planes, dx=None),
        lambda: rg.echo_background_device(planes, dx=400.0, min_dbz="low"),
        lambda: rg.rain_rate_by_class_device(planes, np.zeros((4, 4), np.uint8)),
        lambda: rg.rain_rate_by_class_device(planes, np.zeros((4, 5), np.int32)),
        lambda: rg.rain_rate_by_class_device(planes, np.zeros((4, 5), np.uint8), convective=(0.0, 1.4)),
        lambda: rg.rain_rate_by_class_device(planes, np.zeros((4, 5), np.uint8), stratiform=200.0),
    ]
    for index, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {index} was accepted")
    # one relation with a single class and a zero radius: only the centres themselves are convective
    field = np.full((1, 9, 9), 20.0, np.float32)
    field[0, 4, 4] = 50.0
    got = rg.convective_stratiform(field, dx=400.0, area_relation=((), (0.0,)))
    assert got.sum() == 81 + 1 and got[0, 4, 4] == 2
