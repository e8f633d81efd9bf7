"""Echo motion and nowcasts on the GPU (csrc/rg_motion.hip, radar_processor_amd/motion.py) against the NumPy restatement of
tests/motion_oracle.py on the scenes of tests/motion_scenes.py, through the raw C ABI and through the public functions.

The contract is exact integers plus float64 operations that are rounded once, so nothing here has a tolerance: levels and
integer displacements are equal, nearest samples and bilinear values have the restatement's bits, and a block's score and
motion are the float32 of the restatement's float64 value or that value's float32 neighbour (the one place where two
roundings, float64 then float32, may meet one)."""
import numpy as np
import pytest

import motion_oracle as mo
import motion_scenes as ms
import warp_oracle as wo

pytestmark = pytest.mark.gpu
CANARY = 64                       # elements before and after every output
FILL = -9.25


@pytest.fixture(scope="module")
def env():
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native, motion
    lib = rg.load_library()
    return dict(torch=torch, rg=rg, native=_native, motion=motion, lib=lib, dev=torch.device("cuda", 0))


_PATTERN = {"uint8": 0xA5, "int16": -21555, "float32": -12345.5}


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
    return env["torch"].from_numpy(np.array(a)).to(env["dev"])          # a copy: the scenes' arrays are read-only


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ordered(a):
    """float32 -> int64 that grows with the value, consecutive for neighbouring floats (-0 and +0 coincide)."""
    i = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _assert_rounded(got, want64, what):
    """``got`` float32 holds NaN exactly where ``want64`` does; elsewhere it is float32(want64) or its float32 neighbour."""
    assert np.array_equal(np.isnan(got), np.isnan(want64)), f"{what}: NaN sets differ"
    live = ~np.isnan(want64)
    steps = np.abs(_ordered(got[live]) - _ordered(want64[live].astype(np.float32)))
    assert (steps <= 1).all(), f"{what}: {int((steps > 1).sum())} values lie {int(steps.max())} float32 steps off"


# ---- quantise --------------------------------------------------------------------------------------------------------------
def _quantize_raw(env, src_t, mask_t, shape3, lo, hi, out_t):
    nat = env["native"]
    inv = float(np.float32(254.0 / (hi - lo)))
    with env["torch"].cuda.device(env["dev"]):
        return env["lib"].rg_motion_quantize_f32(nat.ptr(src_t), nat.ptr(mask_t), *shape3, float(np.float32(lo)), inv,
                                                 nat.ptr(out_t), nat.stream_ptr())


FLOAT_SCENES = tuple(n for n in ms.SCENES if n not in ("ties", "degenerate_min_echo"))


@pytest.mark.parametrize("name", FLOAT_SCENES)
def test_quantize_bytes_equal_the_restatement(env, name):
    torch = env["torch"]
    s = ms.scene(name)
    h, w = s.prev.shape[-2:]
    src = np.concatenate([s.prev.reshape(-1, h, w), s.next.reshape(-1, h, w)])           # every plane of the scene
    n = src.shape[0]
    rng = np.random.default_rng(17)
    mask = (rng.random(src.shape) < 0.2).astype(np.uint8) * rng.integers(1, 256, src.shape).astype(np.uint8)
    if s.mask_prev is not None:
        mask[0], mask[1] = s.mask_prev, s.mask_next
    src_t, mask_t = _dev(env, src), _dev(env, mask)
    for m, m_t in ((None, None), (mask, mask_t)):
        buf, out = _guarded(env, (n, h, w), "uint8")
        assert _quantize_raw(env, src_t, m_t, (n, h, w), ms.LO, ms.HI, out) == 0
        torch.cuda.synchronize()
        assert _intact(buf, n * h * w)
        assert np.array_equal(out.cpu().numpy(), mo.quantize(src, ms.LO, ms.HI, m)), (name, m is not None)
    assert src_t.cpu().numpy().tobytes() == src.tobytes() and mask_t.cpu().numpy().tobytes() == mask.tobytes()
    # the public function: other limits, a boolean mask, the rank of the input
    got = env["rg"].quantize_planes_device(src[0], 7.5, 41.0, mask=mask[0] != 0).cpu().numpy()
    assert got.shape == (h, w) and np.array_equal(got, mo.quantize(src[0], 7.5, 41.0, mask[0]))
    assert np.array_equal(env["rg"].quantize_planes_device(src_t).cpu().numpy(), mo.quantize(src))


# ---- block match -----------------------------------------------------------------------------------------------------------
def _match_raw(env, prev_t, next_t, n, h, w, s, min_echo=None):
    """The raw entry point into guarded outputs: ``(status, (disp, motion, score) tensors, their buffers)``."""
    nat = env["native"]
    nby, nbx = (h - s.B) // s.S + 1, (w - s.B) // s.S + 1
    if min_echo is None:
        min_echo = s.B * s.B // 8 if s.min_echo is None else s.min_echo
    bd, disp = _guarded(env, (n, nby, nbx, 2), "int16")
    bm, motion = _guarded(env, (n, nby, nbx, 2), "float32")
    bs, score = _guarded(env, (n, nby, nbx), "float32")
    with env["torch"].cuda.device(env["dev"]):
        status = env["lib"].rg_block_match_u8(nat.ptr(prev_t), nat.ptr(next_t), n, h, w, s.B, s.S, s.R, min_echo, nat.ptr(disp),
                                              nat.ptr(motion), nat.ptr(score), nat.stream_ptr())
    return status, (disp, motion, score), (bd, bm, bs)


@pytest.mark.parametrize("name", ms.SCENES)
def test_block_match_equals_the_restatement_on_every_block(env, name):
    torch = env["torch"]
    s, want = ms.scene(name), ms.match(name)
    qp, qn = ms.levels(name)
    n, nby, nbx = want.valid.shape
    h, w = qp.shape[-2:]
    if name == "stack":                                   # two views of ONE stack of four planes
        stack_t = _dev(env, np.concatenate([qp, qn[-1:]]))
        prev_t, next_t = stack_t[:-1], stack_t[1:]
    else:
        prev_t, next_t = _dev(env, qp), _dev(env, qn)
    status, (disp, motion, score), bufs = _match_raw(env, prev_t, next_t, n, h, w, s)
    assert status == 0
    torch.cuda.synchronize()
    for buf, per in zip(bufs, (2, 2, 1)):
        assert _intact(buf, n * nby * nbx * per)
    assert prev_t.cpu().numpy().tobytes() == np.ascontiguousarray(qp).tobytes()
    assert next_t.cpu().numpy().tobytes() == np.ascontiguousarray(qn).tobytes()
    got_disp, got_motion, got_score = disp.cpu().numpy(), motion.cpu().numpy(), score.cpu().numpy()
    assert np.array_equal(got_disp, want.disp), f"{name}: {int((got_disp != want.disp).any(axis=-1).sum())} blocks differ"
    _assert_rounded(got_score, want.score, f"{name}: score")
    _assert_rounded(got_motion, want.motion, f"{name}: motion")
    assert np.array_equal(np.isnan(got_score), np.isnan(got_motion).all(axis=-1))
    if name == "stack":                                   # ... equals three single-pair calls, bit for bit
        for k in range(n):
            status, single, _ = _match_raw(env, _dev(env, qp[k]), _dev(env, qn[k]), 1, h, w, s)
            assert status == 0
            for a, b in zip(single, (disp, motion, score)):
                assert a[0].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes()
    # the public function from the scene's own planes (quantised on the device, masks applied) gives the same grid
    grid = env["rg"].estimate_motion_device(_dev(env, s.prev), s.next, block=s.B, stride=s.S, search=s.R, lo=ms.LO, hi=ms.HI,
                                            min_echo=s.min_echo, mask_prev=s.mask_prev, mask_next=s.mask_next)
    lead = (n,) if s.prev.ndim == 3 else ()
    assert tuple(grid.motion.shape) == lead + (nby, nbx, 2) and tuple(grid.score.shape) == lead + (nby, nbx)
    assert grid.disp.dtype == torch.int16 and (grid.block, grid.stride, grid.search, grid.shape) == (s.B, s.S, s.R, (h, w))
    assert grid.lattice == mo.block_lattice((h, w), s.B, s.S)
    assert grid.disp.cpu().numpy().tobytes() == got_disp.tobytes()
    assert grid.motion.cpu().numpy().tobytes() == got_motion.tobytes()
    assert grid.score.cpu().numpy().tobytes() == got_score.tobytes()


def test_min_echo_is_the_callers_and_the_default_is_an_eighth_of_the_block(env):
    s = ms.scene("shift")
    qp, qn = ms.levels("shift")
    for min_echo in (1, 100, 256):
        want = mo.block_match(qp, qn, s.B, s.S, s.R, min_echo)
        status, (disp, motion, score), _ = _match_raw(env, _dev(env, qp), _dev(env, qn), 1, *qp.shape, s, min_echo=min_echo)
        assert status == 0
        assert np.array_equal(disp.cpu().numpy(), want.disp)
        _assert_rounded(score.cpu().numpy(), want.score, f"min_echo {min_echo}")
    grid = env["rg"].estimate_motion_device(qp, qn, block=s.B, stride=s.S, search=s.R)       # levels in, the default min_echo
    assert np.array_equal(grid.disp.cpu().numpy(), ms.match("shift").disp[0])


# ---- fill ------------------------------------------------------------------------------------------------------------------
def test_fill_equals_the_restatement_per_plane_pair(env):
    torch, rg = env["torch"], env["rg"]
    s = ms.scene("stack")
    grid = rg.estimate_motion_device(s.prev, s.next, block=s.B, stride=s.S, search=s.R)
    motion, score = grid.motion.cpu().numpy(), grid.score.cpu().numpy()
    assert np.isnan(motion).any()
    for min_score in (0.5, 0.97, 2.0):
        filled = rg.fill_motion_device(grid, min_score)
        assert filled.score is grid.score and filled.disp is grid.disp and filled.lattice == grid.lattice
        got = filled.motion.cpu().numpy()
        assert np.isfinite(got).all()
        for k in range(3):
            assert got[k].tobytes() == mo.fill_motion(motion[k], score[k], min_score).tobytes(), (min_score, k)
        one = rg.fill_motion_device(grid._replace(motion=grid.motion[1], score=grid.score[1], disp=grid.disp[1]), min_score)
        assert tuple(one.motion.shape) == tuple(grid.motion.shape[1:]) and torch.equal(one.motion, filled.motion[1])
    assert not got.any()                                  # min_score 2: none remains, zero


# ---- advect ----------------------------------------------------------------------------------------------------------------
LEADS = (0.0, 1.0, 2.5)
ADVECT_SHAPE = (45, 71)


def _advect_planes():
    """float32 [3, 45, 71]: the rim scene's second plane (NaN holes); a plane that names its pixel, with a NaN that keeps
    its payload and both infinities; smooth values."""
    h, w = ADVECT_SHAPE
    index = wo.index_plane(ADVECT_SHAPE).copy()
    index[7, 9], index[30, 60] = np.inf, -np.inf
    index.view(np.uint32)[20, 33] = 0x7FC12345
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.stack([ms.scene("rim").next, index, (30.0 * np.sin(0.2 * yy) * np.cos(0.13 * xx)).astype(np.float32)])
    out.setflags(write=False)
    return out


def _advect_fields():
    """name -> (float32 motion [ny, nx, 2], Lattice)."""
    h, w = ADVECT_SHAPE
    s, m = ms.scene("rim"), ms.match("rim")
    rim = mo.fill_motion(m.motion[0].astype(np.float32), m.score[0].astype(np.float32), 0.5)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    omega = 0.15                                          # radians per interval about the centre of the plane
    rotation = np.stack([omega * (xx - (w - 1) / 2.0), -omega * (yy - (h - 1) / 2.0)], axis=-1).astype(np.float32)
    row = np.stack([np.linspace(-3.0, 4.0, 6), np.linspace(5.0, -2.5, 6)], axis=-1).astype(np.float32)[None]
    return {"rim": (rim, mo.block_lattice((h, w), s.B, s.S)),
            "one_node": (np.array([[[2.25, -3.5]]], dtype=np.float32), mo.Lattice(20.0, 30.0, 1.0, 1.0, 1, 1)),
            "one_row": (row, mo.Lattice(11.5, 3.25, 2.0, 12.5, 1, 6)),
            "rotation": (rotation, mo.Lattice(0.0, 0.0, 1.0, 1.0, h, w))}


def _advect_raw(env, src_t, n_planes, h, w, field_t, lat, leads, substeps, method, fill, out_t):
    nat = env["native"]
    c_leads = (nat.c_double * max(len(leads), 1))(*leads)
    with env["torch"].cuda.device(env["dev"]):
        return env["lib"].rg_advect_f32(nat.ptr(src_t), n_planes, h, w, nat.ptr(field_t), nat.MotionLattice(*lat), c_leads,
                                        len(leads), substeps, method, fill, nat.ptr(out_t), nat.stream_ptr())


@pytest.mark.parametrize("field_name", ["rim", "one_node", "one_row", "rotation"])
def test_advect_equals_the_restatement_bit_for_bit(env, field_name):
    torch = env["torch"]
    src = _advect_planes()
    P, h, w = src.shape
    field, lat = _advect_fields()[field_name]
    src_t, field_t = _dev(env, src), _dev(env, field)
    for substeps in (1, 4):
        for method in ("nearest", "bilinear"):
            want = mo.advect(src, field, lat, LEADS, substeps, method, FILL)
            buf, out = _guarded(env, (len(LEADS), P, h, w), "float32")
            assert _advect_raw(env, src_t, P, h, w, field_t, lat, LEADS, substeps, env["motion"].ADVECT_METHODS[method], FILL,
                               out) == 0
            torch.cuda.synchronize()
            assert _intact(buf, len(LEADS) * P * h * w)
            got = out.cpu().numpy()
            what = (field_name, substeps, method)
            assert np.array_equal(_bits(got) == _bits(np.float32(FILL)), _bits(want) == _bits(np.float32(FILL))), what
            assert np.array_equal(_bits(got), _bits(want)), f"{what}: {int((_bits(got) != _bits(want)).sum())} values differ"
            assert (got == np.float32(FILL)).any()
            if method == "nearest":
                assert got[0].tobytes() == src.tobytes()  # lead 0 is the source itself
            # three planes in one call are three calls
            for p in range(P):
                single = env["rg"].advect_device(src_t[p], field_t, LEADS, lattice=lat, method=method, substeps=substeps,
                                                 fill_value=FILL)
                assert tuple(single.shape) == (len(LEADS), h, w) and single.cpu().numpy().tobytes() == got[:, p].tobytes()
    assert src_t.cpu().numpy().tobytes() == src.tobytes() and field_t.cpu().numpy().tobytes() == field.tobytes()


def test_advect_surface_stream_out_and_overlap(env):
    torch, rg, nat = env["torch"], env["rg"], env["native"]
    src = _advect_planes()
    P, h, w = src.shape
    s = ms.scene("rim")
    grid = rg.fill_motion_device(rg.estimate_motion_device(s.prev, s.next, block=s.B, stride=s.S, search=s.R))
    field, lat = grid.motion.cpu().numpy(), mo.Lattice(*grid.lattice)
    assert lat == _advect_fields()["rim"][1] and np.isfinite(field).all()
    src_t = _dev(env, src)
    for method in ("nearest", "bilinear"):
        here = rg.advect_device(src_t, grid, LEADS, method=method, substeps=2)     # a MotionGrid carries its lattice
        assert here.cpu().numpy().tobytes() == mo.advect(src, field, lat, LEADS, 2, method).tobytes()
        side = torch.cuda.Stream(device=env["dev"])
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            there = rg.advect_device(src_t, grid, LEADS, method=method, substeps=2)
        side.synchronize()
        assert torch.equal(here.view(torch.int32), there.view(torch.int32))
    # out=: written in place, returned; a single number is one lead; no leads, no launch
    target = torch.full((1, P, h, w), 5.0, dtype=torch.float32, device=env["dev"])
    assert rg.advect_device(src_t, grid, 2.5, fill_value=FILL, out=target) is target
    assert target.cpu().numpy().tobytes() == mo.advect(src, field, lat, (2.5,), 1, "nearest", FILL).tobytes()
    with pytest.raises(ValueError, match="contiguous"):
        rg.advect_device(src_t, grid, 2.5, out=target.double())
    assert tuple(rg.advect_device(src_t, grid, []).shape) == (0, P, h, w)
    # a NaN vector never faults: the pixels it reaches are fill
    holes = _dev(env, field)
    holes[1, 2, 0] = float("nan")
    out = rg.advect_device(src_t[1], holes, [1.0], lattice=lat, fill_value=FILL)
    assert (out == FILL).any() and not (out == FILL).all()
    # out overlapping src is refused, and nothing is written
    both = torch.full((2 * P * h * w,), 3.0, dtype=torch.float32, device=env["dev"])
    for offset in (0, P * h * w - 1):
        status = _advect_raw(env, both, P, h, w, _dev(env, field), lat, (1.0,), 1, 0, 0.0, both[offset:])
        assert status == nat.RG_EINVAL and b"out overlaps src" in env["lib"].rg_last_error()
    torch.cuda.synchronize()
    assert (both == 3.0).all()


# ---- the chain -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(ms.NOWCAST_MOTIONS))
def test_nowcast_equals_the_restatements_chain(env, kind):
    rg = env["rg"]
    frames = ms.nowcast_frames(kind, (0.0, 1.0))
    for method, substeps in (("nearest", 1), ("bilinear", 3)):
        want, filled, m = mo.nowcast(frames[0], frames[1], (1.0, 3.0), ms.B, ms.S, ms.R, method=method, substeps=substeps)
        forecast, grid = rg.nowcast_device(_dev(env, frames[0]), _dev(env, frames[1]), (1.0, 3.0), block=ms.B, stride=ms.S,
                                           search=ms.R, method=method, substeps=substeps)
        assert np.array_equal(grid.disp.cpu().numpy(), m.disp[0])
        assert grid.motion.cpu().numpy().tobytes() == filled.tobytes()
        assert forecast.cpu().numpy().tobytes() == want.tobytes()
    host, host_grid = rg.nowcast(frames[0], frames[1], (1.0, 3.0), block=ms.B, stride=ms.S, search=ms.R, method="bilinear",
                                 substeps=3)
    assert isinstance(host, np.ndarray) and host.tobytes() == want.tobytes() and isinstance(host_grid.motion, np.ndarray)


# ---- the warp still gives its bits -------------------------------------------------------------------------------------------
def test_the_warp_that_shares_the_sampling_code_is_unchanged(env):
    """rg_warp.hip takes its two sampling rules from csrc/rg_sample.hpp now: on one scene of tests/warp_oracle.py the nearest
    samples still equal that oracle bit for bit on every decided pixel, and the bilinear values keep its fill set and lie
    within its bound, for every source."""
    rg = env["rg"]
    name = "rma1_fine"
    s = wo.scene(name)
    src = wo.planes(name, 3)
    got = rg.warp_to_mercator_device(src, s.limits, s.origin, s.raster, device=env["dev"]).cpu().numpy()
    fx, fy, c = wo.mapped(name)
    want = wo.sample_nearest(src, fx, fy, c, s.lattice, np.float32(np.nan))
    decided = ~wo.undecided_nearest(name)
    assert decided.mean() > 0.99 and np.array_equal(_bits(got)[:, decided], _bits(want)[:, decided])
    for kind in wo.BILINEAR_SOURCES:
        d = wo.bilinear_differences(name, kind, env["dev"])
        assert d["fill_set_differs"] == 0 and (d["kept"] <= d["undecided"] or d["worst_excess"] <= 0.0), (kind, d)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_and_leave_outputs_alone(env):
    torch, nat, lib = env["torch"], env["native"], env["lib"]
    s = ms.scene("shift")
    qp, qn = ms.levels("shift")
    h, w = qp.shape
    src_t, qp_t, qn_t = _dev(env, s.prev), _dev(env, qp), _dev(env, qn)
    field, lat = _advect_fields()["one_row"]
    field_t = _dev(env, field)
    bq, q_out = _guarded(env, (1, h, w), "uint8")
    bd, disp = _guarded(env, (1, 6, 9, 2), "int16")
    bm, motion = _guarded(env, (1, 6, 9, 2), "float32")
    bs, score = _guarded(env, (1, 6, 9), "float32")
    ba, adv = _guarded(env, (2, 1, h, w), "float32")
    stream = nat.stream_ptr()
    nan, inf = float("nan"), float("inf")

    def quant(src=nat.ptr(src_t), n=1, hh=h, ww=w, lo=0.0, inv=4.0, dst=nat.ptr(q_out)):
        return lib.rg_motion_quantize_f32(src, None, n, hh, ww, lo, inv, dst, stream)

    def match(prev=nat.ptr(qp_t), nxt=nat.ptr(qn_t), n=1, hh=h, ww=w, B=16, S=8, R=6, e=32, d=nat.ptr(disp), m=nat.ptr(motion),
              sc=nat.ptr(score)):
        return lib.rg_block_match_u8(prev, nxt, n, hh, ww, B, S, R, e, d, m, sc, stream)

    def advect(src=nat.ptr(src_t), n=1, hh=h, ww=w, f=nat.ptr(field_t), lattice=lat, leads=(1.0, 2.0), n_leads=None, k=1, method=0,
               dst=nat.ptr(adv)):
        c_leads = (nat.c_double * 16)(*leads) if leads is not None else None
        return lib.rg_advect_f32(src, n, hh, ww, f, nat.MotionLattice(*lattice), c_leads, len(leads) if n_leads is None else n_leads,
                                 k, method, 0.0, dst, stream)

    def refused(status, word):
        assert status == nat.RG_EINVAL
        assert word in lib.rg_last_error(), lib.rg_last_error()

    with torch.cuda.device(env["dev"]):
        for kw in (dict(src=None), dict(dst=None)):
            refused(quant(**kw), b"rg_motion_quantize_f32: null pointer")
        for kw in (dict(prev=None), dict(nxt=None), dict(d=None), dict(m=None), dict(sc=None)):
            refused(match(**kw), b"rg_block_match_u8: null pointer")
        for kw in (dict(src=None), dict(f=None), dict(dst=None), dict(leads=None, n_leads=1)):
            refused(advect(**kw), b"rg_advect_f32: null pointer")
        for call in (quant, match, advect):
            for n in (0, -1):
                refused(call(n=n), b"at least 1")
            refused(call(hh=-1), b"negative size")
            refused(call(ww=-1), b"negative size")
            refused(call(n=2, hh=1 << 15, ww=1 << 15), b"below 2^31")
        for lo, inv in ((nan, 4.0), (inf, 4.0), (0.0, nan), (0.0, inf)):
            refused(quant(lo=lo, inv=inv), b"must be finite")
        for inv in (0.0, -4.0):
            refused(quant(inv=inv), b"inv_step must be positive")
        for B in (0, 2, 6, 18, 68, -16):
            refused(match(B=B), b"block must be a multiple of 4")
        for S in (0, -8):
            refused(match(S=S), b"stride must be at least 1")
        for R in (-1, 33):
            refused(match(R=R), b"search must lie in")
        for e in (0, 257, -5):
            refused(match(e=e), b"min_echo must lie in")
        refused(match(hh=15), b"smaller than a block")
        refused(match(ww=0), b"smaller than a block")
        refused(advect(leads=(0.0,) * 16, n_leads=17), b"n_leads must lie in")
        refused(advect(n_leads=-1), b"n_leads must lie in")
        for bad in (nan, inf, -inf):
            refused(advect(leads=(1.0, bad)), b"lead 1 is not finite")
            for member in range(4):
                refused(advect(lattice=lat[:member] + (bad,) + lat[member + 1:]), b"rg_motion_lattice is not finite")
        for member in (2, 3):
            for bad in (0.0, -1.0):
                refused(advect(lattice=lat[:member] + (bad,) + lat[member + 1:]), b"must be positive")
        for member in (4, 5):
            for bad in (0, -3):
                refused(advect(lattice=lat[:member] + (bad,) + lat[member + 1:]), b"ny and nx must be at least 1")
        for k in (0, 17, -1):
            refused(advect(k=k), b"substeps must lie in")
        for method in (2, -1):
            refused(advect(method=method), b"unknown method")
        refused(advect(dst=nat.ptr(src_t)), b"out overlaps src")
        refused(advect(src=nat.ptr(adv) + 4 * (2 * h * w - 1)), b"out overlaps src")
        # nothing to do: RG_OK, no launch
        assert quant(hh=0) == 0 and quant(ww=0) == 0 and advect(hh=0) == 0 and advect(ww=0) == 0
        assert advect(leads=(), n_leads=0) == 0 and advect(leads=None, n_leads=0) == 0
    torch.cuda.synchronize()
    for buf in (bq, bd, bm, bs, ba):                      # no refusal, and no empty call, wrote a byte
        assert _untouched(buf)
    assert src_t.cpu().numpy().tobytes() == s.prev.tobytes() and qp_t.cpu().numpy().tobytes() == qp.tobytes()
