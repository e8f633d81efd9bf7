"""The polar-domain phase processing on the device (csrc/rg_phase.hip) against the NumPy restatement of the header
(tests/phase_oracle.py): every scene of tests/phase_scenes.py through the raw C ABI between canaries and through the public
functions, EQUAL on the bits of every output at every gate (NaN payloads count) -- the sums are integers, the float steps are
stated one by one, so there is no tolerance.  Each call is repeated into dirtied outputs and must reproduce."""
import ctypes

import numpy as np
import pytest

import phase_oracle as po
import phase_scenes as ps

pytestmark = pytest.mark.gpu

CANARY = 64                       # elements before and after every output
_PATTERN = {"int32": -1234567, "float32": -12345.5, "uint16": 0xA5A5}
RG_EINVAL = -1


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
    host = np.full(n + 2 * CANARY, _PATTERN[dtype], dtype=dtype)
    buf = torch.from_numpy(host).to(env["dev"])
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


def _equal(got, want, what):
    np.testing.assert_array_equal(po.bits(got.cpu().numpy()), po.bits(want), err_msg=str(what))


def _scale(s):
    return 500.0 / (65536.0 * s.spacing)


# ---- the raw calls -------------------------------------------------------------------------------------------------------------
def _run_unfold(env, s, want_folds=True):
    """Twice into the same guarded outputs (the second time they hold the first result's neighbours and a new pattern)."""
    lib, P = env["lib"], env["native"].ptr
    R, G = s.phidp.shape
    src, mask = _dev(env, s.phidp), _dev(env, s.mask)
    out_buf, out = _guarded(env, (R, G), "float32")
    folds_buf, folds = _guarded(env, (R, G), "int32") if want_folds else (None, None)
    for attempt in range(2):
        if attempt:
            out.fill_(-7.25)
            if want_folds:
                folds.fill_(99)
        status = lib.rg_phidp_unfold_f32(P(src), P(mask), R, G, s.wrap, P(out), P(folds), env["native"].stream_ptr())
        assert status == 0, lib.rg_last_error().decode()
        want_out, want_folds_a = po.unfold(s.phidp, s.mask, s.wrap)
        _equal(out, want_out, "out")
        assert _intact(out_buf, R * G)
        if want_folds:
            _equal(folds, want_folds_a, "folds")
            assert _intact(folds_buf, R * G)
    return out


def _run_fit(env, s, skip=()):
    lib, P = env["lib"], env["native"].ptr
    R, G = s.phi.shape
    phi, dbz = _dev(env, s.phi), _dev(env, s.dbz)
    bufs = {name: _guarded(env, (R, G), dtype) for name, dtype in (("kdp", "float32"), ("phi_s", "float32"), ("count", "uint16"))
            if name not in skip}
    view = {name: bufs[name][1] if name in bufs else None for name in ("kdp", "phi_s", "count")}
    edges = (ctypes.c_double * max(len(s.edges), 1))(*s.edges)
    half = (ctypes.c_int32 * len(s.half_window))(*s.half_window)
    want = po.fit(s.phi, _scale(s), half_window=s.half_window, min_valid=s.min_valid, dbz=s.dbz, edges=s.edges,
                  centre_only=s.centre_only)
    for attempt in range(2):
        if attempt:
            for name, (_, v) in bufs.items():
                v.copy_(env["torch"].full_like(v.cpu(), 77).to(env["dev"]))
        status = lib.rg_phidp_fit_f32(P(phi), R, G, P(dbz), edges, half, len(s.half_window), s.min_valid, int(s.centre_only), _scale(s),
                                      P(view["kdp"]), P(view["phi_s"]), P(view["count"]), env["native"].stream_ptr())
        assert status == 0, lib.rg_last_error().decode()
        for name, (buf, v) in bufs.items():
            _equal(v, getattr(want, name), name)
            assert _intact(buf, R * G), name
    return want


def _run_attenuation(env, s, skip=(), in_place=False):
    lib, P = env["lib"], env["native"].ptr
    R, G = s.phi_s.shape
    phi, phi0 = _dev(env, s.phi_s), _dev(env, s.phi0)
    want = po.attenuation(s.phi_s, s.dbz, alpha=s.alpha, beta=s.beta, max_dphi=s.max_dphi, zdr=s.zdr, phi0=s.phi0)
    names = [n for n in ("dbz", "zdr", "pia", "dphi") if n not in skip and not (n == "zdr" and s.zdr is None)]
    bufs = {name: _guarded(env, (R, G), "float32") for name in names}
    view = {name: bufs[name][1] if name in bufs else None for name in ("dbz", "zdr", "pia", "dphi")}
    for attempt in range(2):
        if in_place:                                          # the inputs stand in the guarded outputs
            view["dbz"].copy_(_dev(env, s.dbz))
            dbz = view["dbz"]
            zdr = None
            if s.zdr is not None:
                view["zdr"].copy_(_dev(env, s.zdr))
                zdr = view["zdr"]
            for name in ("pia", "dphi"):
                if attempt and view[name] is not None:
                    view[name].fill_(3.5)
        else:
            dbz, zdr = _dev(env, s.dbz), _dev(env, s.zdr)
            if attempt:
                for v in view.values():
                    if v is not None:
                        v.fill_(3.5)
        status = lib.rg_attenuation_phidp_f32(P(phi), P(phi0), R, G, s.alpha, s.beta, s.max_dphi, P(dbz), P(zdr), P(view["dbz"]),
                                              P(view["zdr"]), P(view["pia"]), P(view["dphi"]), env["native"].stream_ptr())
        assert status == 0, lib.rg_last_error().decode()
        for name, (buf, v) in bufs.items():
            _equal(v, getattr(want, name), name)
            assert _intact(buf, R * G), name


@pytest.mark.parametrize("name", sorted(ps.unfold_scenes()))
def test_unfold_scene_through_the_c_abi(env, name):
    _run_unfold(env, ps.unfold_scenes()[name])


def test_unfold_without_mask_without_folds_and_in_place(env):
    s = ps.unfold_scenes()["seams"]
    _run_unfold(env, s._replace(mask=None), want_folds=False)
    lib, P = env["lib"], env["native"].ptr
    R, G = s.phidp.shape
    buf, data = _guarded(env, (R, G), "float32")
    data.copy_(_dev(env, s.phidp))
    assert lib.rg_phidp_unfold_f32(P(data), P(_dev(env, s.mask)), R, G, s.wrap, P(data), None, env["native"].stream_ptr()) == 0
    _equal(data, po.unfold(s.phidp, s.mask, s.wrap)[0], "in place")
    assert _intact(buf, R * G)


@pytest.mark.parametrize("name", sorted(ps.fit_scenes()))
def test_fit_scene_through_the_c_abi(env, name):
    _run_fit(env, ps.fit_scenes()[name])


@pytest.mark.parametrize("skip", [("kdp",), ("phi_s",), ("count",), ("kdp", "count"), ("phi_s", "count")])
def test_fit_with_each_optional_output_null(env, skip):
    _run_fit(env, ps.fit_scenes()["fit_5x129"], skip=skip)
    _run_fit(env, ps.fit_scenes()["gaps"]._replace(dbz=None), skip=skip)


def test_fit_both_ways_about_the_centre(env):
    for name in ("fit_9x200", "fit_5x65", "sparse", "limits"):
        s = ps.fit_scenes()[name]
        _run_fit(env, s._replace(centre_only=not s.centre_only))


def test_fit_across_tiles(env):
    """Rays of 1300 gates: three tiles of 512 with a partial last one, windows of 255 reaching across both tile seams."""
    rng = np.random.default_rng(77)
    phi = (50.0 + np.cumsum(rng.uniform(0.0, 1.0, (3, 1300)), axis=1) + rng.normal(0.0, 3.0, (3, 1300))).astype(np.float32)
    phi[rng.random(phi.shape) < 0.2] = np.nan
    phi[1, 500:530] = np.nan
    dbz = rng.uniform(0.0, 60.0, phi.shape).astype(np.float32)
    _run_fit(env, ps.Fit(phi, dbz, ps.EDGES4, (255, 100, 20, 1), 5, False, 240.0))
    _run_fit(env, ps.Fit(phi, None, (), (255,), 5, True, 240.0))


@pytest.mark.parametrize("name", sorted(ps.attenuation_scenes()))
def test_attenuation_scene_through_the_c_abi(env, name):
    _run_attenuation(env, ps.attenuation_scenes()[name])


@pytest.mark.parametrize("name", ["paths", "paths_phi0", "att_5x129"])
def test_attenuation_in_place_and_with_optional_outputs_null(env, name):
    s = ps.attenuation_scenes()[name]
    _run_attenuation(env, s, in_place=True)
    _run_attenuation(env, s, skip=("pia",))
    _run_attenuation(env, s, skip=("dphi",), in_place=True)
    _run_attenuation(env, s._replace(zdr=None), skip=("pia", "dphi"))


def test_rays_beyond_one_launch_row(env):
    """4099 rays of 3 gates: 1025 workgroups of four rays with a partial last one, and as many tiles for the fit."""
    rng = np.random.default_rng(5)
    phi = rng.uniform(-180.0, 180.0, (4099, 3)).astype(np.float32)
    phi[rng.random(phi.shape) < 0.2] = np.nan
    _run_unfold(env, ps.Unfold(phi, None, 360.0))
    _run_fit(env, ps.Fit(phi, None, (), (1,), 2, False, 100.0))
    _run_attenuation(env, ps.Attenuation(phi, None, phi.copy(), None, 0.1, 0.0, 50.0))


# ---- refusals leave the outputs alone --------------------------------------------------------------------------------------------
def test_refusals_leave_the_canaried_outputs_untouched(env):
    lib, P, stream = env["lib"], env["native"].ptr, env["native"].stream_ptr()
    R, G = 5, 65
    src = _dev(env, ps.unfold_scenes()["ramp_5x65"].phidp)
    a_buf, a = _guarded(env, (R, G), "float32")
    b_buf, b = _guarded(env, (R, G), "float32")
    i_buf, i = _guarded(env, (R, G), "int32")
    c_buf, c = _guarded(env, (R, G), "uint16")
    half = (ctypes.c_int32 * 1)(5)
    nan = float("nan")
    calls = [
        lambda: lib.rg_phidp_unfold_f32(P(src), None, R, G, 0.0, P(a), P(i), stream),
        lambda: lib.rg_phidp_unfold_f32(P(src), None, R, G, nan, P(a), P(i), stream),
        lambda: lib.rg_phidp_unfold_f32(P(src), None, 0, G, 360.0, P(a), P(i), stream),
        lambda: lib.rg_phidp_unfold_f32(P(src), None, R, 32769, 360.0, P(a), P(i), stream),
        lambda: lib.rg_phidp_unfold_f32(None, None, R, G, 360.0, P(a), P(i), stream),
        lambda: lib.rg_phidp_unfold_f32(P(src), None, R, G, 360.0, P(a), P(a) + 8, stream),
        lambda: lib.rg_phidp_fit_f32(P(src), R, G, None, None, half, 1, 1, 0, 1.0, P(a), P(b), P(c), stream),
        lambda: lib.rg_phidp_fit_f32(P(src), R, G, None, None, half, 2, 3, 0, 1.0, P(a), P(b), P(c), stream),
        lambda: lib.rg_phidp_fit_f32(P(src), R, G, None, None, half, 1, 3, 0, nan, P(a), P(b), P(c), stream),
        lambda: lib.rg_phidp_fit_f32(P(src), R, G, None, None, half, 1, 3, 0, 1.0, None, None, P(c), stream),
        lambda: lib.rg_phidp_fit_f32(P(src), R, G, None, None, half, 1, 3, 0, 1.0, P(a), P(a) + 4, P(c), stream),
        lambda: lib.rg_attenuation_phidp_f32(P(src), None, R, G, -1.0, 0.0, 360.0, P(src), None, P(a), None, P(b), None, stream),
        lambda: lib.rg_attenuation_phidp_f32(P(src), None, R, G, 0.1, 0.0, 0.0, P(src), None, P(a), None, P(b), None, stream),
        lambda: lib.rg_attenuation_phidp_f32(P(src), None, R, G, 0.1, 0.0, 360.0, P(src), P(src), P(a), None, P(b), None, stream),
        lambda: lib.rg_attenuation_phidp_f32(P(src), None, R, G, 0.1, 0.0, 360.0, P(src), None, P(src), None, P(b), None, stream),
        lambda: lib.rg_attenuation_phidp_f32(P(src), None, R, G, 0.1, 0.0, 360.0, P(a), None, P(a), None, P(a), P(b), stream),
    ]
    for n, call in enumerate(calls):
        assert call() == RG_EINVAL, n
    env["torch"].cuda.synchronize()
    for buf in (a_buf, b_buf, i_buf, c_buf):
        assert _untouched(buf)
    assert lib.rg_phidp_unfold_f32(P(src), None, R, 0, 360.0, P(a), P(i), stream) == 0            # nothing to do: no launch
    env["torch"].cuda.synchronize()
    assert _untouched(a_buf) and _untouched(i_buf)


# ---- the public functions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["seams", "seams_180", "ramp_9x200", "ramp_1x1", "ramp_5x63"])
def test_unfold_device_function(env, name):
    rg, s = env["rg"], ps.unfold_scenes()[name]
    want = po.unfold(*s)
    out, folds = rg.unfold_phidp_device(_dev(env, s.phidp), mask=_dev(env, s.mask), wrap=s.wrap, return_folds=True)
    _equal(out, want[0], "out")
    _equal(folds, want[1], "folds")
    again = rg.unfold_phidp_device(s.phidp, mask=s.mask.astype(bool), wrap=s.wrap)              # ndarrays, a mask of another type
    _equal(again, want[0], "from ndarrays")


@pytest.mark.parametrize("name", ["fit_9x200", "fit_5x129", "fit_1x2", "l255", "sparse", "gaps_centre"])
def test_fit_device_function(env, name):
    rg, s = env["rg"], ps.fit_scenes()[name]
    want = po.fit(s.phi, _scale(s), half_window=s.half_window, min_valid=s.min_valid, dbz=s.dbz, edges=s.edges,
                  centre_only=s.centre_only)
    half = s.half_window[0] if len(s.half_window) == 1 else s.half_window
    got = rg.fit_phidp_device(_dev(env, s.phi), s.spacing, half_window=half, min_valid=s.min_valid, dbz=_dev(env, s.dbz),
                              dbz_edges=s.edges, centre_only=s.centre_only)
    assert isinstance(got, rg.PhaseFit) and str(got.count.dtype) == "torch.uint16"
    _equal(got.kdp, want.kdp, "kdp")
    _equal(got.phidp, want.phi_s, "phidp")
    _equal(got.count, want.count, "count")


@pytest.mark.parametrize("name", ["paths", "paths_phi0", "att_9x200", "att_1x1"])
def test_correct_attenuation_device_function(env, name):
    rg, s = env["rg"], ps.attenuation_scenes()[name]
    want = po.attenuation(s.phi_s, s.dbz, alpha=s.alpha, beta=s.beta, max_dphi=s.max_dphi, zdr=s.zdr, phi0=s.phi0)
    got = rg.correct_attenuation_device(_dev(env, s.phi_s), _dev(env, s.dbz), zdr=_dev(env, s.zdr), alpha=s.alpha, beta=s.beta,
                                        phi0=_dev(env, s.phi0), max_dphi=s.max_dphi)
    assert isinstance(got, rg.AttenuationCorrection) and (got.zdr is None) == (s.zdr is None)
    for field in ("dbz", "pia", "dphi") + (("zdr",) if s.zdr is not None else ()):
        _equal(getattr(got, field), getattr(want, field), field)
    one = rg.correct_attenuation_device(s.phi_s, s.dbz, alpha=s.alpha, beta=s.beta, phi0=12.5, max_dphi=s.max_dphi)
    _equal(one.dphi, po.attenuation(s.phi_s, s.dbz, alpha=s.alpha, beta=s.beta, max_dphi=s.max_dphi,
                                    phi0=np.full(s.phi_s.shape[0], 12.5, np.float32)).dphi, "a number for phi0")


def test_rays_without_gates_come_back_empty(env):
    """[R, 0] is legal in the C ABI (RG_OK without a launch); an empty tensor has no address, so the wrappers make no call."""
    rg, torch = env["rg"], env["torch"]
    empty = torch.empty((3, 0), dtype=torch.float32, device=env["dev"])
    out, folds = rg.unfold_phidp_device(empty, mask=torch.empty((3, 0), dtype=torch.uint8, device=env["dev"]), return_folds=True)
    assert tuple(out.shape) == tuple(folds.shape) == (3, 0) and folds.dtype == torch.int32
    fit = rg.fit_phidp_device(empty, 240.0)
    assert all(tuple(t.shape) == (3, 0) for t in fit) and fit.count.dtype == torch.uint16
    corr = rg.correct_attenuation_device(empty, empty, zdr=empty, alpha=0.08, beta=0.02)
    assert all(tuple(t.shape) == (3, 0) for t in corr)
    host = rg.process_phase(np.zeros((3, 0), np.float32), np.zeros((3, 0), np.float32), 240.0)
    assert all(a.shape == (3, 0) for a in host if a is not None) and host.zdr is None and host.dbz.dtype == np.float32


def test_the_chain_on_the_weather_scene_equals_the_three_oracle_stages(env):
    rg, w = env["rg"], ps.weather()
    rhohv_mask = (np.random.default_rng(3).random(w.phidp.shape) < 0.03).astype(np.uint8)
    alpha, beta = rg.ATTENUATION_COEFFICIENTS["C"]
    unfolded, _ = po.unfold(w.phidp, rhohv_mask, 360.0)
    for edges, half, phi0 in (((), 15, None), ((35.0, 48.0), (20, 10, 5), w.offset)):     # the origin found, and the offset given
        hw = (half,) if isinstance(half, int) else half
        origin = None if phi0 is None else np.full(w.phidp.shape[0], phi0, np.float32)
        fit = po.fit(unfolded, 500.0 / (65536.0 * w.spacing), half_window=hw, min_valid=8, dbz=w.dbz if edges else None, edges=edges)
        att = po.attenuation(fit.phi_s, w.dbz, alpha=alpha, beta=beta, max_dphi=360.0, zdr=w.zdr, phi0=origin)
        want = dict(phidp_unfolded=unfolded, phidp=fit.phi_s, kdp=fit.kdp, count=fit.count, dbz=att.dbz, zdr=att.zdr, pia=att.pia,
                    dphi=att.dphi)
        got = rg.process_phase_device(_dev(env, w.phidp), _dev(env, w.dbz), w.spacing, zdr=_dev(env, w.zdr), mask=_dev(env, rhohv_mask),
                                      band="C", half_window=half, min_valid=8, dbz_edges=edges, phi0=phi0)
        assert isinstance(got, rg.PhaseProducts)
        for field, value in want.items():
            _equal(getattr(got, field), value, field)
        host = rg.process_phase(w.phidp, w.dbz, w.spacing, zdr=w.zdr, mask=rhohv_mask, band="C", half_window=half, min_valid=8,
                                dbz_edges=edges, phi0=phi0)
        for field, value in want.items():
            got_host = getattr(host, field)
            assert isinstance(got_host, np.ndarray) and got_host.dtype == value.dtype
            np.testing.assert_array_equal(po.bits(got_host), po.bits(value), err_msg=field)
    # what the stage is for: the corrected field is close to the unattenuated one behind the cells, the raw one is not
    behind = (slice(None), slice(200, 300))
    assert np.abs(w.dbz[behind] - w.dbz_true[behind]).mean() > 10.0
    assert np.abs(host.dbz[behind] - w.dbz_true[behind]).mean() < 0.5
