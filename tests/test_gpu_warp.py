"""The Web Mercator warp and the overview pyramid on the GPU (csrc/rg_warp.hip) against the float64 restatements of
tests/warp_oracle.py: nearest samples bit for bit on every decided pixel of every scene (float planes and RGBA, which must
name the same source pixel), bilinear values within the derived bound and with the oracle's fill set, both overview rules,
memory discipline (canaries, untouched inputs, another stream), the refusals of the four C entry points, and
``web_mercator_rgba`` against the composition of its pieces.

The bilinear bound is ``|got - float32(want)| <= ulp_f32(want) + 2 * (1e-6 m / min(step_x, step_y)) * D``: 1e-6 m is the
plane-coordinate floor derived in tests/test_gpu_georef.py; divided by the step it is the coordinate error in nodes, taken
once per axis; D is the largest difference between two finite taps of one cell (1001 for the ``iy * 1000 + ix`` sources).
Measured on an MI355X (profiles/warp_bounds.json): every pixel of every scene and source within the bound; the figures are in
that file."""
import json

import numpy as np
import pytest

import warp_oracle as wo
from conftest import load_golden

pytestmark = pytest.mark.gpu
CANARY = 64                       # elements before and after every output
PATTERN = -12345.5
PATTERN_U32 = 0xA5C3F00F


@pytest.fixture(scope="module")
def env():
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native, georef
    lib = rg.load_library()
    return dict(torch=torch, rg=rg, native=_native, georef=georef, lib=lib, dev=torch.device("cuda", 0))


def _guarded_f32(env, shape):
    n = int(np.prod(shape))
    buf = env["torch"].full((n + 2 * CANARY,), PATTERN, dtype=env["torch"].float32, device=env["dev"])
    return buf, buf[CANARY:CANARY + n].view(shape)


def _guarded_rgba(env, h, w):
    """uint8 [h, w, 4] inside a buffer of 32-bit canaries (the image stays 4-byte aligned)."""
    torch = env["torch"]
    buf = torch.full((h * w + 2 * CANARY,), PATTERN_U32 - (1 << 32), dtype=torch.int32, device=env["dev"])
    return buf, buf[CANARY:CANARY + h * w].view(torch.uint8).view(h, w, 4)


def _intact(buf, n):
    host = buf.cpu().numpy()
    edge = np.concatenate([host[:CANARY], host[CANARY + n:]])
    return bool((edge == edge.dtype.type(PATTERN if edge.dtype == np.float32 else PATTERN_U32 - (1 << 32))).all())


def _structs(env, s: wo.Scene):
    nat = env["native"]
    return nat.WarpSource(*s.lattice), env["georef"].make_georef(s.origin, s.origin), nat.MercatorRaster(*s.raster)


def _warp_f32(env, s, src_t, n_planes, method, fill, out_t):
    nat = env["native"]
    source, georef, raster = _structs(env, s)
    with env["torch"].cuda.device(env["dev"]):
        return env["lib"].rg_warp_mercator_f32(nat.ptr(src_t), n_planes, source, georef, raster, method, fill, nat.ptr(out_t),
                                               nat.stream_ptr())


def _warp_rgba(env, s, src_t, out_t):
    nat = env["native"]
    source, georef, raster = _structs(env, s)
    with env["torch"].cuda.device(env["dev"]):
        return env["lib"].rg_warp_mercator_rgba8(nat.ptr(src_t), source, georef, raster, nat.ptr(out_t), nat.stream_ptr())


def _dev(env, a):
    return env["torch"].from_numpy(np.array(a)).to(env["dev"])          # a copy: the oracle's arrays are read-only


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_nearest(name, got, src, fill):
    """Decided pixels equal the oracle bit for bit; an undecided pixel equals one of its candidates."""
    s = wo.scene(name)
    fx, fy, c = wo.mapped(name)
    want = wo.sample_nearest(src, fx, fy, c, s.lattice, fill)
    und = wo.undecided_nearest(name)
    if src.dtype == np.uint8:
        same = (got == want).all(axis=-1)
        assert same[~und].all(), f"{name}: {int((~same[~und]).sum())} decided RGBA pixels differ"
        either = np.any([(got == cand).all(axis=-1) for cand in wo.nearest_candidates(name, src, fill)], axis=0)
    else:
        same = _bits(got) == _bits(want)
        assert same[:, ~und].all(), f"{name}: {int((~same[:, ~und]).sum())} decided pixels differ"
        either = np.any([_bits(got) == _bits(cand) for cand in wo.nearest_candidates(name, src, fill)], axis=0).all(axis=0)
    assert either[und].all()


# ---- nearest ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wo.SCENES)
def test_nearest_float_planes_and_rgba_name_the_oracles_source_pixel(env, name):
    torch = env["torch"]
    s = wo.scene(name)
    h, w = s.raster.height, s.raster.width
    plane0 = None
    for n_planes, fill in ((1, np.float32(-7.5)), (3, np.float32(np.nan))):
        src = wo.planes(name, n_planes)
        src_t = _dev(env, src)
        buf, out = _guarded_f32(env, (n_planes, h, w))
        assert _warp_f32(env, s, src_t, n_planes, 0, float(fill), out) == 0
        torch.cuda.synchronize()
        assert _intact(buf, n_planes * h * w)
        assert src_t.cpu().numpy().tobytes() == src.tobytes()                  # the input is untouched
        got = out.cpu().numpy()
        _assert_nearest(name, got, src, fill)
        if n_planes == 1:
            plane0 = got[0]
        else:                                                                  # one coordinate evaluation for all planes
            inside = plane0 != np.float32(-7.5)
            assert np.array_equal(got[0][inside], plane0[inside]) and np.isnan(got[:, ~inside]).all()
            assert np.array_equal(np.isnan(got[0]), ~inside)
    # the RGBA route
    rgba = wo.index_rgba(s.shape)
    rgba_t = _dev(env, rgba)
    buf, out = _guarded_rgba(env, h, w)
    assert _warp_rgba(env, s, rgba_t, out) == 0
    torch.cuda.synchronize()
    assert _intact(buf, h * w) and rgba_t.cpu().numpy().tobytes() == rgba.tobytes()
    got = out.cpu().numpy()
    _assert_nearest(name, got, rgba, 0)
    # ... names the same source pixel as the float route, everywhere
    opaque = got[..., 3] == 255
    assert np.array_equal(opaque, plane0 != np.float32(-7.5)) and not got[~opaque].any()
    named = got[..., 0].astype(np.float32) * np.float32(1000.0) + got[..., 1].astype(np.float32)
    assert np.array_equal(named[opaque], plane0[opaque])


def test_the_far_hemisphere_is_fill_although_it_lands_inside_the_plane(env):
    s = wo.scene("far_hemisphere")
    fx, fy, c = wo.mapped("far_hemisphere")
    got = env["rg"].warp_to_mercator_device(wo.planes("far_hemisphere", 1)[0], s.limits, s.origin, s.raster,
                                            fill_value=-1.0, device=env["dev"]).cpu().numpy()
    beyond = c >= wo.LIMIT + wo.ANGLE_EPS
    assert beyond.mean() > 0.5 and (got[beyond] == -1.0).all()
    assert (got[c < wo.LIMIT - wo.ANGLE_EPS] >= 0.0).all()                    # every visible pixel carries a source value


def test_python_surface_ranks_out_and_another_stream(env):
    torch, rg = env["torch"], env["rg"]
    s = wo.scene("rma1_fine")
    h, w = s.raster.height, s.raster.width
    src = wo.planes("rma1_fine", 3)
    kw = dict(grid_limits=((0.0, 1.0),) + s.limits, grid_origin=s.origin + (431.0,), raster=rg.MercatorRaster(*s.raster))
    three = rg.warp_to_mercator_device(src, device=env["dev"], **kw)
    one = rg.warp_to_mercator_device(_dev(env, src[0]), **kw)
    assert three.shape == (3, h, w) and one.shape == (h, w) and three.dtype == one.dtype == torch.float32
    assert torch.equal(three[0].view(torch.int32), one.view(torch.int32))
    _assert_nearest("rma1_fine", three.cpu().numpy(), src, np.float32(np.nan))
    rgba = rg.warp_to_mercator_device(wo.index_rgba(s.shape), device=env["dev"], **kw)
    assert rgba.shape == (h, w, 4) and rgba.dtype == torch.uint8
    _assert_nearest("rma1_fine", rgba.cpu().numpy(), wo.index_rgba(s.shape), 0)
    # out=: written in place, returned
    target = torch.full((3, h, w), 5.0, dtype=torch.float32, device=env["dev"])
    assert rg.warp_to_mercator_device(src, out=target, fill_value=-3.25, **kw) is target
    assert torch.equal(target.isnan() | (target == -3.25), three.isnan())
    with pytest.raises(ValueError, match="contiguous"):
        rg.warp_to_mercator_device(src, out=target.double(), **kw)
    # a non-default stream gives the same bits, for both methods
    src_t = _dev(env, src)
    for method in ("nearest", "bilinear"):
        here = rg.warp_to_mercator_device(src_t, method=method, **kw)
        side = torch.cuda.Stream(device=env["dev"])
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            there = rg.warp_to_mercator_device(src_t, method=method, **kw)
            levels = rg.overview_pyramid_device(there, [2, 16], "average")
        side.synchronize()
        assert torch.equal(here.view(torch.int32), there.view(torch.int32))
        for a, b in zip(levels, rg.overview_pyramid_device(here, [2, 16], "average")):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- bilinear --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wo.SCENES)
def test_bilinear_against_the_float64_restatement(env, name):
    torch = env["torch"]
    s = wo.scene(name)
    h, w = s.raster.height, s.raster.width
    for kind in wo.BILINEAR_SOURCES:
        d = wo.bilinear_differences(name, kind, env["dev"])
        print(f"{name} / {kind}: {json.dumps(d)}")
        assert d["pixels"] == s.pixels and d["undecided"] <= wo.UNDECIDED_CAP * s.pixels
        assert d["fill_set_differs"] == 0, f"{name} / {kind}: {d['fill_set_differs']} decided pixels are fill on one side only"
        if d["kept"] > d["undecided"]:
            assert d["worst_excess"] <= 0.0, f"{name} / {kind}: a value lies {d['worst_excess']} beyond the bound"
    # the four sources as planes of ONE call, a finite fill, canaries: each plane is its own single-plane call, bit for bit
    stack = np.stack([wo.bilinear_source(name, kind) for kind in wo.BILINEAR_SOURCES])
    stack_t = _dev(env, stack)
    buf, out = _guarded_f32(env, (4, h, w))
    assert _warp_f32(env, s, stack_t, 4, 1, -9.25, out) == 0
    torch.cuda.synchronize()
    assert _intact(buf, 4 * h * w) and stack_t.cpu().numpy().tobytes() == stack.tobytes()
    got = out.cpu().numpy()
    for k in range(4):
        single = env["rg"].warp_to_mercator_device(stack[k], s.limits, s.origin, s.raster, method="bilinear",
                                                   device=env["dev"]).cpu().numpy()
        assert np.array_equal(got[k] == np.float32(-9.25), np.isnan(single))
        keep = ~np.isnan(single)
        assert np.array_equal(_bits(got[k])[keep], _bits(single)[keep])


def test_bilinear_keeps_an_echo_edge_where_nearest_keeps_it(env):
    """A half-plane of echo: bilinear with the 0.5 rule fills exactly the pixels nearest fills, decisions on the edge aside
    (the two rules cut at the same line when three of four taps are present or absent together)."""
    s = wo.scene("rma1_fine")
    plane = wo.index_plane(s.shape).copy()
    plane[:, 20:] = np.nan
    kw = dict(grid_limits=s.limits, grid_origin=s.origin, raster=s.raster, device=env["dev"])
    near = np.isnan(env["rg"].warp_to_mercator_device(plane, **kw).cpu().numpy())
    bil = np.isnan(env["rg"].warp_to_mercator_device(plane, method="bilinear", **kw).cpu().numpy())
    fx, fy, c = wo.mapped("rma1_fine")
    inner = (fy > 0.0) & (fy < s.shape[0] - 1.0) & (fx > 0.0)        # away from the plane's own rim, where bilinear loses taps
    edge = np.abs(fx - 19.5) < 2e-6
    assert inner.sum() > 10000 and np.array_equal(near[inner & ~edge], bil[inner & ~edge])


# ---- overviews -------------------------------------------------------------------------------------------------------------
def _overview_f32(env, src_t, n_planes, h, w, f, method, out_t):
    nat = env["native"]
    with env["torch"].cuda.device(env["dev"]):
        return env["lib"].rg_overview_f32(nat.ptr(src_t), n_planes, h, w, f, method, nat.ptr(out_t), nat.stream_ptr())


def _overview_rgba(env, src_t, h, w, f, out_t):
    nat = env["native"]
    with env["torch"].cuda.device(env["dev"]):
        return env["lib"].rg_overview_rgba8(nat.ptr(src_t), h, w, f, nat.ptr(out_t), nat.stream_ptr())


@pytest.mark.parametrize("name", wo.MAIN)
def test_overview_levels_against_the_restatement(env, name):
    torch = env["torch"]
    img = wo.overview_input(name)
    _, h, w = img.shape
    img_t = _dev(env, img)
    rng = np.random.default_rng(5)
    rgba = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    rgba_t = _dev(env, rgba)
    for f in wo.FACTORS:
        oh, ow = wo.overview_shape(h, w, f)
        for method in (0, 1):
            buf, out = _guarded_f32(env, (2, oh, ow))
            assert _overview_f32(env, img_t, 2, h, w, f, method, out) == 0
            torch.cuda.synchronize()
            assert _intact(buf, 2 * oh * ow)
            got = out.cpu().numpy()
            if method == 0:
                assert np.array_equal(_bits(got), _bits(wo.overview_nearest(img, f))), (name, f)
            else:
                want = wo.overview_average(img, f)
                assert np.array_equal(np.isnan(got), np.isnan(want)), (name, f)
                live = ~np.isnan(want)
                err = np.abs(got[live].astype(np.float64) - want[live].astype(np.float32))
                assert (err <= wo.ulp_f32(want[live])).all(), (name, f, float(err.max()))
                assert np.isfinite(got[live]).all()                                    # +-inf never reach a mean
        buf, out = _guarded_rgba(env, oh, ow)
        assert _overview_rgba(env, rgba_t, h, w, f, out) == 0
        torch.cuda.synchronize()
        assert _intact(buf, oh * ow) and np.array_equal(out.cpu().numpy(), wo.overview_nearest(rgba, f)), (name, f)
    assert img_t.cpu().numpy().tobytes() == img.tobytes() and rgba_t.cpu().numpy().tobytes() == rgba.tobytes()
    # what the inputs were built to hold: blocks without a finite value, and one with a single finite value
    avg16 = env["rg"].overview_pyramid_device(img_t, [16], "average")[0].cpu().numpy()
    assert np.isnan(avg16[0, 0, 0]) and avg16[0, 1, 1] == np.float32(42.5)


def test_pyramid_surface(env):
    torch, rg = env["torch"], env["rg"]
    img = wo.index_plane((37, 53))
    levels = rg.overview_pyramid_device(img, device=env["dev"])                 # None: [2, 4, 8, 16]
    assert [tuple(t.shape) for t in levels] == [(19, 27), (10, 14), (5, 7), (3, 4)]
    for f, t in zip((2, 4, 8, 16), levels):
        assert np.array_equal(t.cpu().numpy(), wo.overview_nearest(img, f))
    top, = rg.overview_pyramid_device(img, [64], device=env["dev"])             # 64 on 37 x 53: one pixel
    assert tuple(top.shape) == (1, 1) and float(top[0, 0]) == 32032.0
    mean, = rg.overview_pyramid_device(_dev(env, img), [64], " Average")
    assert tuple(mean.shape) == (1, 1) and float(mean[0, 0]) == np.float32(img.astype(np.float64).mean())
    stack = rg.overview_pyramid_device(np.stack([img, -img]), [4], "average", device=env["dev"])[0]
    assert tuple(stack.shape) == (2, 10, 14) and torch.equal(stack[1], -stack[0])
    rgba = wo.index_rgba((37, 53))
    r8, = rg.overview_pyramid_device(rgba, [8], device=env["dev"])
    assert r8.dtype == torch.uint8 and np.array_equal(r8.cpu().numpy(), wo.overview_nearest(rgba, 8))
    assert rg.overview_pyramid_device(_dev(env, img), []) == []


# ---- the C entry points' refusals ------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_and_leave_outputs_alone(env):
    torch, nat, lib = env["torch"], env["native"], env["lib"]
    s = wo.scene("rma1")
    h, w = s.raster.height, s.raster.width
    src_t = _dev(env, wo.planes("rma1", 1))
    rgba_t = _dev(env, wo.index_rgba(s.shape))
    buf, out = _guarded_f32(env, (1, h, w))
    rbuf, rout = _guarded_rgba(env, h, w)
    good = _structs(env, s)
    stream = nat.stream_ptr()

    def f32(src=nat.ptr(src_t), n=1, source=good[0], g=good[1], raster=good[2], method=0, dst=nat.ptr(out)):
        return lib.rg_warp_mercator_f32(src, n, source, g, raster, method, 0.0, dst, stream)

    def rgba8(src=nat.ptr(rgba_t), source=good[0], g=good[1], raster=good[2], dst=nat.ptr(rout)):
        return lib.rg_warp_mercator_rgba8(src, source, g, raster, dst, stream)

    def ov(src=nat.ptr(src_t), n=1, hh=s.shape[0], ww=s.shape[1], f=2, method=0, dst=nat.ptr(out)):
        return lib.rg_overview_f32(src, n, hh, ww, f, method, dst, stream)

    def ov8(src=nat.ptr(rgba_t), hh=s.shape[0], ww=s.shape[1], f=2, dst=nat.ptr(rout)):
        return lib.rg_overview_rgba8(src, hh, ww, f, dst, stream)

    def refused(status, word, code=nat.RG_EINVAL):
        assert status == code
        msg = lib.rg_last_error()
        assert word in msg, msg

    with torch.cuda.device(env["dev"]):
        for kw in (dict(src=None), dict(source=None), dict(g=None), dict(raster=None), dict(dst=None)):
            refused(f32(**kw), b"rg_warp_mercator_f32: null pointer")
            refused(rgba8(**kw), b"rg_warp_mercator_rgba8: null pointer")
        for kw in (dict(src=None), dict(dst=None)):
            refused(ov(**kw), b"rg_overview_f32: null pointer")
            refused(ov8(**kw), b"rg_overview_rgba8: null pointer")
        for n in (0, -1):
            refused(f32(n=n), b"n_planes must be at least 1")
            refused(ov(n=n), b"n_planes must be at least 1")
        for method in (2, -1):
            refused(f32(method=method), b"unknown method")
            refused(ov(method=method), b"unknown method")
        for f in (1, 0, 65, -2):
            refused(ov(f=f), b"factor must lie in 2 .. 64")
            refused(ov8(f=f), b"factor must lie in 2 .. 64")
        refused(ov(hh=-1), b"negative size")
        refused(ov8(ww=-1), b"negative size")

        def changed(kind, **members):
            fresh = _structs(env, s)[kind]
            for k, v in members.items():
                setattr(fresh, k, v)
            return fresh

        for member in ("x_lo", "y_lo", "step_x", "step_y"):
            for bad in (np.nan, np.inf):
                refused(f32(source=changed(0, **{member: bad})), b"rg_warp_source is not finite")
                refused(rgba8(source=changed(0, **{member: bad})), b"rg_warp_source is not finite")
        for member in ("step_x", "step_y"):
            for bad in (0.0, -1.0):
                refused(f32(source=changed(0, **{member: bad})), b"must be positive")
        for member in ("ny", "nx"):
            for bad in (1, 0, -5):
                refused(f32(source=changed(0, **{member: bad})), b"at least 2")
                refused(rgba8(source=changed(0, **{member: bad})), b"at least 2")
        for member, _ in nat.Georef._fields_[:-2]:
            for bad in (np.nan, np.inf) + ((0.0, -1.0) if member == "radius" else ()):
                refused(f32(g=changed(1, **{member: bad})), b"radius" if member == "radius" else b"rg_georef is not finite")
        for member in ("x_min", "y_max", "pixel"):
            for bad in (np.nan, -np.inf):
                refused(f32(raster=changed(2, **{member: bad})), b"rg_mercator_raster is not finite")
                refused(rgba8(raster=changed(2, **{member: bad})), b"rg_mercator_raster is not finite")
        for bad in (0.0, -3.0):
            refused(f32(raster=changed(2, pixel=bad)), b"pixel must be positive")
        refused(f32(raster=changed(2, width=-1)), b"negative width or height")
        refused(rgba8(raster=changed(2, height=-1)), b"negative width or height")
        # out overlapping src: the same array, or any shared byte
        refused(f32(dst=nat.ptr(src_t)), b"out overlaps src")
        refused(f32(dst=nat.ptr(src_t) + 4 * (s.shape[0] * s.shape[1] - 1)), b"out overlaps src")
        refused(f32(src=nat.ptr(out) + 4 * (h * w - 1)), b"out overlaps src")
        refused(rgba8(dst=nat.ptr(rgba_t)), b"out overlaps src")
        refused(ov(dst=nat.ptr(src_t)), b"out overlaps src")
        refused(ov8(dst=nat.ptr(rgba_t) + 8), b"out overlaps src")
        refused(rgba8(dst=nat.ptr(rout) + 2), b"4-byte aligned", nat.RG_EALIGN)
        refused(ov8(src=nat.ptr(rgba_t) + 1), b"4-byte aligned", nat.RG_EALIGN)
        # nothing to do: RG_OK, no launch
        assert f32(raster=changed(2, width=0)) == 0 and f32(raster=changed(2, height=0)) == 0
        assert rgba8(raster=changed(2, width=0)) == 0 and ov(hh=0) == 0 and ov8(ww=0) == 0
    torch.cuda.synchronize()
    # no refusal, and no empty call, wrote a byte
    assert (buf.cpu().numpy() == np.float32(PATTERN)).all() and (rbuf.cpu().numpy() == PATTERN_U32 - (1 << 32)).all()
    assert src_t.cpu().numpy().tobytes() == wo.planes("rma1", 1).tobytes()


# ---- the chain -------------------------------------------------------------------------------------------------------------
LUT_COLOURS = np.stack([np.linspace(0.0, 1.0, 16), np.linspace(1.0, 0.2, 16), np.full(16, 0.5), np.ones(16)], axis=1)


@pytest.mark.parametrize("method,resampling", [("nearest", "nearest"), ("bilinear", "average"), ("nearest", "average")])
def test_web_mercator_rgba_is_the_composition_of_its_pieces(env, method, resampling):
    torch, rg = env["torch"], env["rg"]
    s = wo.scene("lat_70")
    plane = wo.bilinear_source("lat_70", "nan_30_percent")
    lut = rg.colormap_lut(LUT_COLOURS)
    vmin, vmax = 2000.0, 30000.0
    raster, rgba, levels = rg.web_mercator_rgba(plane, s.limits, s.origin, lut, vmin, vmax, method=method,
                                                resampling=resampling, device=env["dev"])
    assert raster == rg.mercator_raster_for(s.shape, s.limits, s.origin) == s.raster and isinstance(raster, rg.MercatorRaster)
    warped = rg.warp_to_mercator_device(plane, s.limits, s.origin, raster, method=method, device=env["dev"])
    want = rg.colormap_rgba_device(warped, lut, vmin, vmax)
    assert rgba.dtype == torch.uint8 and tuple(rgba.shape) == (raster.height, raster.width, 4) and torch.equal(rgba, want)
    assert rgba[..., 3].any() and not rgba[..., 3].all()                          # echo and no echo
    if resampling == "average":
        pieces = [rg.colormap_rgba_device(t, lut, vmin, vmax) for t in rg.overview_pyramid_device(warped, None, "average")]
    else:
        pieces = rg.overview_pyramid_device(want, None, "nearest")
    assert len(levels) == 4 and all(torch.equal(a, b) for a, b in zip(levels, pieces))
    # a raster of the caller's, other factors
    tile = rg.mercator_tile(5, 16, 7, size=96)
    r2, rgba2, levels2 = rg.web_mercator_rgba(_dev(env, plane), s.limits, s.origin, lut, vmin, vmax, raster=tile, method=method,
                                              factors=[3, 64], resampling=resampling)
    assert r2 == tile and tuple(rgba2.shape) == (96, 96, 4) and [tuple(t.shape) for t in levels2] == [(32, 32, 4), (2, 2, 4)]
    assert rg.web_mercator_rgba(plane, s.limits, s.origin, lut, vmin, vmax, factors=[], device=env["dev"])[2] == []


def test_end_to_end_from_a_golden_grid(env):
    """tests/golden/g5_products_z15.npz: the stored grid -> COLMAX on the device -> onto the map.  The plane is the
    fixture's own COLMAX; the image is the oracle's nearest warp of it through the colormap kernel, byte for byte."""
    torch, rg = env["torch"], env["rg"]
    _, arrays = load_golden("g5_products_z15")
    colmax = rg.column_max(arrays["grid"])
    assert np.array_equal(colmax, arrays["P_colmax"], equal_nan=True)
    ny, nx = colmax.shape
    limits, origin = ((0.0, 15000.0), (-117e3, 117e3), (-165e3, 165e3)), wo.RMA1 + (476.0,)
    lut = rg.colormap_lut(LUT_COLOURS)
    live = colmax[np.isfinite(colmax)]
    vmin, vmax = float(live.min()), float(live.max())
    plane = np.ascontiguousarray(colmax, dtype=np.float32)
    raster, rgba, levels = rg.web_mercator_rgba(plane, limits, origin, lut, vmin, vmax, device=env["dev"])
    assert raster == rg.mercator_raster_for((20, ny, nx), limits, origin)
    Xg, Yg, c = wo.pixel_map(wo.Raster(*raster), origin[:2])
    lat = wo.lattice((ny, nx), limits[1:])
    fx, fy = wo.node_coords(Xg, Yg, lat)
    und = wo._near_integer(fx + 0.5, wo.EDGE_EPS) | wo._near_integer(fy + 0.5, wo.EDGE_EPS)
    assert und.sum() <= wo.UNDECIDED_CAP * und.size
    warped = wo.sample_nearest(plane[None], fx, fy, c, lat, np.nan)[0]
    want = rg.colormap_rgba_device(_dev(env, warped), lut, vmin, vmax).cpu().numpy()
    got = rgba.cpu().numpy()
    assert np.array_equal(got[~und], want[~und]) and got[..., 3].any()
    assert [tuple(t.shape) for t in levels] == [(-(-raster.height // f), -(-raster.width // f), 4) for f in (2, 4, 8, 16)]
    for f, t in zip((2, 4, 8, 16), levels):
        assert np.array_equal(t.cpu().numpy(), wo.overview_nearest(got, f))
