"""Rain rate and advection-corrected accumulation on the GPU (csrc/rg_accumulate.hip, radar_processor_amd/accumulation.py)
against the NumPy restatement of tests/accumulation_oracle.py on the scenes of tests/accumulation_scenes.py, through the raw C
ABI between canaries and through the public functions.

The accumulation is float64 operations that are rounded once each, on samples that are the advection's own bits, so nothing
about it has a tolerance: ``out`` and ``out_steps`` are equal to the restatement bit for bit, and on two scenes also to the
composition of ``rg_advect_f32`` launches blended in NumPy, a yardstick that shares nothing with the restatement but the
blend rule.  The rate's classes are exact; elsewhere a value is the restatement's float32 or its float32 neighbour -- the
argument of ``exp`` has the same bits on both sides, each library's ``exp`` lies within 1 ulp(float64) of the true value, so
the two float64 results lie within 2 ulp of each other and their float32 roundings within one float32 step."""
import numpy as np
import pytest

import accumulation_oracle as ao
import accumulation_scenes as sc
import motion_oracle as mo

pytestmark = pytest.mark.gpu
CANARY = 64                       # elements before and after every output
_PATTERN = {"uint8": 0xA5, "float32": -12345.5}


@pytest.fixture(scope="module")
def env():
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native, motion
    lib = rg.load_library()
    return dict(torch=torch, rg=rg, native=_native, motion=motion, lib=lib, dev=torch.device("cuda", 0))


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


def _same(got, want):
    """NaN in the same places (a sum's NaN has no agreed payload) and the same bits elsewhere."""
    live = ~np.isnan(want)
    return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(_bits(got)[live], _bits(want)[live])


def _method(env, s):
    return env["motion"].ADVECT_METHODS[s.method]


def _accumulate_raw(env, prev_t, next_t, shape3, field_t, lat, hours, n_steps, substeps, method, min_steps, fill, out_t, steps_t):
    nat = env["native"]
    with env["torch"].cuda.device(env["dev"]):
        return env["lib"].rg_accumulate_advected_f32(nat.ptr(prev_t), nat.ptr(next_t), *shape3, nat.ptr(field_t),
                                                     nat.MotionLattice(*lat), hours, n_steps, substeps, method, min_steps, fill,
                                                     nat.ptr(out_t), nat.ptr(steps_t), nat.stream_ptr())


def _scene_tensors(env, s):
    prev_t = _dev(env, s.prev)
    return prev_t, (prev_t if s.next is s.prev else _dev(env, s.next)), _dev(env, s.motion)


# ---- the accumulation against the restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.SCENES)
def test_accumulation_equals_the_restatement_bit_for_bit(env, name):
    torch, rg = env["torch"], env["rg"]
    s, want = sc.scene(name), sc.expected(name)
    shape3 = s.prev.shape
    n = s.prev.size
    prev_t, next_t, field_t = _scene_tensors(env, s)
    bo, out = _guarded(env, shape3, "float32")
    bs, steps = _guarded(env, shape3, "uint8")
    assert _accumulate_raw(env, prev_t, next_t, shape3, field_t, s.lattice, s.hours, s.n_steps, s.substeps, _method(env, s),
                           s.min_steps, s.fill, out, steps) == 0
    torch.cuda.synchronize()
    assert _intact(bo, n) and _intact(bs, n)
    got, got_steps = out.cpu().numpy(), steps.cpu().numpy()
    assert np.array_equal(got_steps, want.steps), f"{name}: {int((got_steps != want.steps).sum())} counts differ"
    assert np.array_equal(sc.is_fill(got, s.fill), sc.is_fill(want.out, s.fill)), name
    assert np.array_equal(_bits(got), _bits(want.out)), f"{name}: {int((_bits(got) != _bits(want.out)).sum())} of {n} values differ"
    assert prev_t.cpu().numpy().tobytes() == s.prev.tobytes() and next_t.cpu().numpy().tobytes() == s.next.tobytes()
    assert field_t.cpu().numpy().tobytes() == s.motion.tobytes()
    # without out_steps: the same plane
    bo2, out2 = _guarded(env, shape3, "float32")
    assert _accumulate_raw(env, prev_t, next_t, shape3, field_t, s.lattice, s.hours, s.n_steps, s.substeps, _method(env, s),
                           s.min_steps, s.fill, out2, None) == 0
    torch.cuda.synchronize()
    assert _intact(bo2, n) and out2.cpu().numpy().tobytes() == got.tobytes()
    # the public function: tensors or arrays in, the planes' own rank out, every plane on its own the same
    kw = dict(steps=s.n_steps, lattice=s.lattice, method=s.method, substeps=s.substeps, min_steps=s.min_steps, fill_value=s.fill)
    depth, count = rg.accumulate_device(prev_t, s.next, field_t, s.hours, return_steps=True, **kw)
    assert depth.cpu().numpy().tobytes() == got.tobytes() and count.cpu().numpy().tobytes() == got_steps.tobytes()
    for p in range(shape3[0]):
        single = rg.accumulate_device(prev_t[p], next_t[p], s.motion, s.hours, **kw)
        assert tuple(single.shape) == shape3[1:] and single.cpu().numpy().tobytes() == got[p].tobytes(), (name, p)


def test_public_surface_out_default_min_steps_zero_motion_and_arrays(env):
    torch, rg = env["torch"], env["rg"]
    s, want = sc.scene("zero_motion"), sc.expected("zero_motion")
    prev_t, next_t, _ = _scene_tensors(env, s)
    # motion=None is zero motion; min_steps defaults to steps; out= is written and returned
    target = torch.full(s.prev.shape, 5.0, dtype=torch.float32, device=env["dev"])
    assert rg.accumulate_device(prev_t, next_t, None, s.hours, steps=s.n_steps, fill_value=s.fill, out=target) is target
    assert target.cpu().numpy().tobytes() == want.out.tobytes()
    with pytest.raises(ValueError, match="contiguous"):
        rg.accumulate_device(prev_t, next_t, None, s.hours, steps=s.n_steps, out=target.double())
    host = rg.accumulate(s.prev, s.next, None, s.hours, steps=s.n_steps, fill_value=s.fill)
    assert isinstance(host, np.ndarray) and host.tobytes() == want.out.tobytes()
    host, count = rg.accumulate(s.prev, s.next, None, s.hours, steps=s.n_steps, fill_value=s.fill, return_steps=True)
    assert isinstance(count, np.ndarray) and count.dtype == np.uint8 and np.array_equal(count, want.steps)
    # a MotionGrid carries its lattice
    b = sc.scene("six_planes")
    grid = env["motion"].MotionGrid(_dev(env, b.motion), None, None, 8, 4, 4, b.prev.shape[-2:], b.lattice.origin_y, b.lattice.step_y)
    depth = rg.accumulate_device(b.prev, b.next, grid, b.hours, steps=b.n_steps, method=b.method, min_steps=b.min_steps)
    assert depth.cpu().numpy().tobytes() == sc.expected("six_planes").out.tobytes()
    # the moving pixel leaves its swath on the device too
    prev, nxt, motion, lat = sc.moving_pixel()
    out = rg.accumulate(prev, nxt, motion, sc.MOVING_HOURS, steps=8, lattice=lat, method="nearest")[0]
    assert sorted(zip(*np.nonzero(out))) == [(2, x) for x in range(5, 13)]
    assert out.astype(np.float64).sum() == sc.MOVING_RATE * sc.MOVING_HOURS
    # a NaN vector never faults: the samples it reaches are missing
    s = sc.scene("dense_nearest")
    holes = _dev(env, s.motion)
    holes[5, 7, 0] = float("nan")
    out = rg.accumulate_device(s.prev, s.next, holes, s.hours, steps=s.n_steps, method="nearest", fill_value=sc.FILL).cpu().numpy()
    assert out[0, 5, 7] == np.float32(sc.FILL)
    elsewhere = np.ones(out.shape, dtype=bool)
    elsewhere[0, 4:6, 6:8] = False                        # the pixels whose interpolant holds node (5, 7), with weight 0 too
    assert np.array_equal(_bits(out)[elsewhere], _bits(sc.expected("dense_nearest").out)[elsewhere])


# ---- the accumulation against the composition of rg_advect_f32 ---------------------------------------------------------------
@pytest.mark.parametrize("name", sc.COMPOSED)
def test_accumulation_equals_the_composition_of_the_advection_kernel(env, name):
    """The other yardstick: every sample taken by ``advect_device`` (the kernel this one fuses) at the leads ``s`` and
    ``s - 1`` with a NaN fill, blended and summed here in NumPy float64 by the header's rule."""
    rg = env["rg"]
    s = sc.scene(name)
    prev_t, next_t, field_t = _scene_tensors(env, s)
    leads = [(float(k) + 0.5) / float(s.n_steps) for k in range(s.n_steps)]
    kw = dict(lattice=s.lattice, method=s.method, substeps=s.substeps, fill_value=float("nan"))
    a_all, b_all = [], []
    for lo in range(0, s.n_steps, 16):                    # at most 16 leads per launch
        a_all.append(rg.advect_device(prev_t, field_t, leads[lo:lo + 16], **kw).cpu().numpy())
        b_all.append(rg.advect_device(next_t, field_t, [v - 1.0 for v in leads[lo:lo + 16]], **kw).cpu().numpy())
    a_all, b_all = np.concatenate(a_all), np.concatenate(b_all)
    total, n = np.zeros(s.prev.shape), np.zeros(s.prev.shape, dtype=np.int64)
    for k, lead in enumerate(leads):
        a, b = a_all[k].astype(np.float64), b_all[k].astype(np.float64)
        has_a, has_b = ~np.isnan(a), ~np.isnan(b)
        with np.errstate(invalid="ignore"):
            r = np.where(has_a & has_b, (1.0 - lead) * a + lead * b, np.where(has_a, a, b))
        total = np.where(has_a | has_b, total + np.where(has_a | has_b, r, 0.0), total)
        n += has_a | has_b
    with np.errstate(invalid="ignore", divide="ignore"):
        depth = (s.hours * (total / np.maximum(n, 1).astype(np.float64))).astype(np.float32)
    want = np.where(n >= s.min_steps, depth, np.float32(s.fill)).astype(np.float32)
    got, count = rg.accumulate_device(prev_t, next_t, field_t, s.hours, steps=s.n_steps, lattice=s.lattice, method=s.method,
                                      substeps=s.substeps, min_steps=s.min_steps, fill_value=s.fill, return_steps=True)
    assert np.array_equal(count.cpu().numpy(), n.astype(np.uint8))
    assert 0 < (n < s.min_steps).sum() < n.size and (n == s.n_steps).any()
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), f"{name}: {int((_bits(got.cpu().numpy()) != _bits(want)).sum())} differ"


# ---- the rate ----------------------------------------------------------------------------------------------------------------
def _rate_planes():
    """float32 dBZ ``[3, 37, 53]`` from -20 to 75 with NaN, both infinities, and the limits themselves; a mask of any byte."""
    rng = np.random.default_rng(23)
    src = rng.uniform(-20.0, 75.0, (3, 37, 53)).astype(np.float32)
    src[rng.random(src.shape) < 0.1] = np.nan
    flat = src.reshape(-1)
    flat[:8] = (5.0, np.nextafter(np.float32(5.0), np.float32(0.0)), 55.0, np.nextafter(np.float32(55.0), np.float32(99.0)), np.inf,
                -np.inf, 0.0, -0.0)
    mask = (rng.random(src.shape) < 0.15).astype(np.uint8) * rng.integers(1, 256, src.shape).astype(np.uint8)
    mask.reshape(-1)[:8] = 0
    return src, mask


@pytest.mark.parametrize("relation", [(200.0, 1.6, 5.0, 55.0), (300.0, 1.4, -10.0, 70.0)])
def test_rain_rate_classes_are_exact_and_values_within_one_float32_step(env, relation):
    torch, nat, rg = env["torch"], env["native"], env["rg"]
    a, b, min_dbz, max_dbz = relation
    src, mask = _rate_planes()
    src_t, mask_t = _dev(env, src), _dev(env, mask)
    p, q = ao.zr_constants(a, b)
    for m, m_t in ((None, None), (mask, mask_t)):
        want = ao.rain_rate(src, a, b, min_dbz, max_dbz, m)
        buf, out = _guarded(env, src.shape, "float32")
        with torch.cuda.device(env["dev"]):
            assert env["lib"].rg_rain_rate_f32(nat.ptr(src_t), nat.ptr(m_t), *src.shape, p, q, min_dbz, max_dbz, nat.ptr(out),
                                               nat.stream_ptr()) == 0
        torch.cuda.synchronize()
        assert _intact(buf, src.size)
        got = out.cpu().numpy()
        none = np.isnan(src) | (False if m is None else m != 0)
        dry = ~none & ~(src >= np.float32(min_dbz))
        capped = ~none & (src >= np.float32(max_dbz))
        assert none.any() and dry.any() and capped.any() and (~none & ~dry & ~capped).any()
        assert (_bits(got)[none] == ao.NAN_BITS).all() and np.array_equal(np.isnan(got), none)
        assert (_bits(got)[dry] == 0).all()                                   # +0.0
        assert (got[capped] == got[capped][0]).all() and np.isfinite(got[capped][0])
        wet = ~none & ~dry
        steps = np.abs(_ordered(got[wet]) - _ordered(want[wet]))
        print(f"rain rate {relation}, mask {m is not None}: {int((steps != 0).sum())} of {int(wet.sum())} values are not identical, "
              f"the furthest {int(steps.max())} float32 step(s) off")
        assert (steps <= 1).all(), f"{int((steps > 1).sum())} values lie more than one float32 step off (up to {int(steps.max())})"
        assert (got[wet] > 0.0).all()
    assert src_t.cpu().numpy().tobytes() == src.tobytes() and mask_t.cpu().numpy().tobytes() == mask.tobytes()
    # the public function: a boolean mask, the rank of the input
    one = rg.rain_rate_device(src[1], a=a, b=b, min_dbz=min_dbz, max_dbz=max_dbz, mask=mask[1] != 0)
    assert tuple(one.shape) == src.shape[1:] and one.cpu().numpy().tobytes() == got[1].tobytes()
    assert tuple(rg.rain_rate_device(src_t, a=a, b=b, min_dbz=min_dbz, max_dbz=max_dbz).shape) == src.shape


# ---- streams -----------------------------------------------------------------------------------------------------------------
def test_a_side_stream_gives_the_same_bits(env):
    torch, rg = env["torch"], env["rg"]
    s = sc.scene("dense_bilinear")
    prev_t, next_t, field_t = _scene_tensors(env, s)
    src, mask = _rate_planes()
    src_t = _dev(env, src)
    kw = dict(steps=s.n_steps, lattice=s.lattice, method=s.method, substeps=s.substeps, min_steps=s.min_steps, return_steps=True)
    here, here_steps = rg.accumulate_device(prev_t, next_t, field_t, s.hours, **kw)
    here_rate = rg.rain_rate_device(src_t)
    side = torch.cuda.Stream(device=env["dev"])
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        bo, out = _guarded(env, s.prev.shape, "float32")
        bs, steps = _guarded(env, s.prev.shape, "uint8")
        assert _accumulate_raw(env, prev_t, next_t, s.prev.shape, field_t, s.lattice, s.hours, s.n_steps, s.substeps,
                               _method(env, s), s.min_steps, float("nan"), out, steps) == 0
        there, there_steps = rg.accumulate_device(prev_t, next_t, field_t, s.hours, **kw)
        there_rate = rg.rain_rate_device(src_t)
    side.synchronize()
    assert _intact(bo, s.prev.size) and _intact(bs, s.prev.size)
    assert torch.equal(here.view(torch.int32), there.view(torch.int32)) and torch.equal(here_steps, there_steps)
    assert torch.equal(here.view(torch.int32), out.view(torch.int32)) and torch.equal(here_steps, steps)
    assert torch.equal(here_rate.view(torch.int32), there_rate.view(torch.int32))
    assert here.cpu().numpy().tobytes() == sc.expected("dense_bilinear").out.tobytes()


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_and_leave_outputs_alone(env):
    torch, nat, lib = env["torch"], env["native"], env["lib"]
    s = sc.scene("block_sub3")
    P, h, w = s.prev.shape
    lat = tuple(s.lattice)
    prev_t, next_t, field_t = _scene_tensors(env, s)
    src_t = _dev(env, s.prev)
    br, rate = _guarded(env, (P, h, w), "float32")
    bo, out = _guarded(env, (P, h, w), "float32")
    bs, steps = _guarded(env, (P, h, w), "uint8")
    stream = nat.stream_ptr()
    nan, inf = float("nan"), float("inf")

    def rain(src=nat.ptr(src_t), n=P, hh=h, ww=w, p=0.14, q=3.3, lo=5.0, hi=55.0, dst=nat.ptr(rate)):
        return lib.rg_rain_rate_f32(src, None, n, hh, ww, p, q, lo, hi, dst, stream)

    def acc(prev=nat.ptr(prev_t), nxt=nat.ptr(next_t), n=P, hh=h, ww=w, f=nat.ptr(field_t), lattice=lat, hours=0.1, k=4, sub=1,
            method=1, least=2, dst=nat.ptr(out), cnt=nat.ptr(steps)):
        return lib.rg_accumulate_advected_f32(prev, nxt, n, hh, ww, f, nat.MotionLattice(*lattice), hours, k, sub, method, least, 0.0,
                                              dst, cnt, stream)

    def refused(status, word):
        assert status == nat.RG_EINVAL
        assert word in lib.rg_last_error(), lib.rg_last_error()

    with torch.cuda.device(env["dev"]):
        for kw in (dict(src=None), dict(dst=None)):
            refused(rain(**kw), b"rg_rain_rate_f32: null pointer")
        for kw in (dict(prev=None), dict(nxt=None), dict(f=None), dict(dst=None)):
            refused(acc(**kw), b"rg_accumulate_advected_f32: null pointer")
        for call in (rain, acc):
            for n in (0, -1):
                refused(call(n=n), b"at least 1")
            refused(call(hh=-1), b"negative size")
            refused(call(ww=-1), b"negative size")
            refused(call(n=2, hh=1 << 15, ww=1 << 15), b"below 2^31")
        for p in (nan, inf, -inf, 0.0, -0.14):
            refused(rain(p=p), b"p must be finite and positive")
        for kw in (dict(q=nan), dict(q=inf), dict(lo=nan), dict(lo=-inf), dict(hi=nan), dict(hi=inf)):
            refused(rain(**kw), b"must be finite")
        refused(rain(lo=30.0, hi=29.0), b"max_dbz lies below min_dbz")
        for bad in (nan, inf, -inf):
            for member in range(4):
                refused(acc(lattice=lat[:member] + (bad,) + lat[member + 1:]), b"rg_motion_lattice is not finite")
            refused(acc(hours=bad), b"hours must be finite and positive")
        for member in (2, 3):
            for bad in (0.0, -1.0):
                refused(acc(lattice=lat[:member] + (bad,) + lat[member + 1:]), b"must be positive")
        for member in (4, 5):
            for bad in (0, -3):
                refused(acc(lattice=lat[:member] + (bad,) + lat[member + 1:]), b"ny and nx must be at least 1")
        for hours in (0.0, -0.25):
            refused(acc(hours=hours), b"hours must be finite and positive")
        for k in (0, 65, -1):
            refused(acc(k=k, least=1), b"n_steps must lie in")
        for sub in (0, 17, -1):
            refused(acc(sub=sub), b"substeps must lie in")
        for method in (2, -1):
            refused(acc(method=method), b"unknown method")
        for least in (0, 5, -1):
            refused(acc(least=least), b"min_steps must lie in")
        for inp in (prev_t, next_t, field_t):
            refused(acc(dst=nat.ptr(inp)), b"out overlaps an input")
            refused(acc(cnt=nat.ptr(inp) + 5), b"out_steps overlaps an input")
        refused(acc(prev=nat.ptr(out) + 4 * (P * h * w - 1)), b"out overlaps an input")
        refused(acc(nxt=nat.ptr(steps) + (P * h * w - 1)), b"out_steps overlaps an input")
        refused(acc(cnt=nat.ptr(out) + 4 * (P * h * w) - 1), b"out_steps overlaps out")
        # nothing to do: RG_OK, no launch
        assert rain(hh=0) == 0 and rain(ww=0) == 0 and acc(hh=0) == 0 and acc(ww=0) == 0
    torch.cuda.synchronize()
    for buf in (br, bo, bs):                              # no refusal, and no empty call, wrote a byte
        assert _untouched(buf)
    assert prev_t.cpu().numpy().tobytes() == s.prev.tobytes() and field_t.cpu().numpy().tobytes() == s.motion.tobytes()
    # the limits themselves are taken
    with torch.cuda.device(env["dev"]):
        assert acc(k=64, least=64, sub=16, method=0) == 0 and acc(k=1, least=1) == 0 and rain(lo=30.0, hi=30.0) == 0
    torch.cuda.synchronize()
    assert _intact(bo, P * h * w) and _intact(bs, P * h * w) and _intact(br, P * h * w)


# ---- the accumulator ---------------------------------------------------------------------------------------------------------
def test_rain_accumulator_follows_a_moving_cell(env):
    torch, rg = env["torch"], env["rg"]
    frames = sc.frames(4)
    h, w = sc.FRAME_SHAPE
    dt = sc.FRAME_SECONDS
    corner = np.zeros((h, w), dtype=np.uint8)
    corner[0:6, 0:8] = 1                                  # not seen in the first two scans, far from the cell
    lat = mo.block_lattice((h, w), sc.FRAME_ESTIMATE["block"], sc.FRAME_ESTIMATE["stride"])
    steps = sc.FRAME_ESTIMATE["search"]
    acc = rg.RainAccumulator(window_seconds=2 * dt, **sc.FRAME_ESTIMATE)
    assert acc.steps == steps and acc.total() is None
    rates, intervals, ends = [], [], []
    for t in range(4):
        mask = corner if t < 2 else None
        frame = acc.update(_dev(env, frames[t]) if t % 2 else frames[t], t * dt, mask=mask)
        rate = frame.rate.cpu().numpy()
        want_rate = ao.rain_rate(frames[t], mask=mask)
        assert np.array_equal(np.isnan(rate), np.isnan(want_rate)) and np.array_equal(rate == 0.0, want_rate == 0.0)
        wet = want_rate > 0.0
        assert wet.any() and (np.abs(_ordered(rate[wet]) - _ordered(want_rate[wet])) <= 1).all()
        rates.append(rate)
        if t == 0:
            assert frame.interval_mm is None and frame.total_mm is None and frame.motion is None and frame.seconds is None
            continue
        assert frame.seconds == dt and tuple(frame.motion.lattice) == tuple(lat)
        field = frame.motion.motion.cpu().numpy()                          # the tracker's own filled motion, read back
        assert field.shape == (lat.ny, lat.nx, 2) and np.isfinite(field).all()
        want = ao.accumulate(rates[t - 1][None], rate[None], field, lat, dt / 3600.0, steps, 1, "bilinear").out[0]
        got = frame.interval_mm.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want)), (t, int((_bits(got) != _bits(want)).sum()))
        intervals.append(got)
        ends.append(t * dt)
        want_total = ao.window_total(intervals, ends, t * dt, 2 * dt)
        assert _same(frame.total_mm.cpu().numpy(), want_total), t
        assert len(acc.intervals) == min(t, 2)                             # the window drops the oldest interval
    assert _same(want_total, (intervals[1].astype(np.float64) + intervals[2].astype(np.float64)).astype(np.float32))
    assert _same(acc.total(window_seconds=dt).cpu().numpy(), intervals[2])
    # the first interval joined two scans that did not see the corner: NaN there, and NaN in every sum that holds it ...
    assert np.isnan(intervals[0][:3, :4]).all() and not np.isnan(intervals[1][:3, 3:6]).any()
    again = rg.RainAccumulator(window_seconds=3600.0, **sc.FRAME_ESTIMATE)
    for t in range(3):
        last = again.update(frames[t], t * dt, mask=corner if t < 2 else None)
    assert last.interval_mm.cpu().numpy().tobytes() == intervals[1].tobytes()
    total = last.total_mm.cpu().numpy()
    assert _same(total, ao.window_total(intervals[:2], ends[:2], 2 * dt, 3600.0))
    assert np.array_equal(np.isnan(total), np.isnan(intervals[0]) | np.isnan(intervals[1]))
    # ... unless skip_missing: then it adds nothing
    kept = again.total(skip_missing=True).cpu().numpy()
    assert np.array_equal(_bits(kept), _bits(ao.window_total(intervals[:2], ends[:2], 2 * dt, 3600.0, skip_missing=True)))
    only_first = np.isnan(intervals[0]) & ~np.isnan(intervals[1])
    assert not np.isnan(kept).any() and only_first.sum() > 10 and np.array_equal(kept[only_first], intervals[1][only_first])
    assert np.array_equal(_bits(kept[~np.isnan(total)]), _bits(total[~np.isnan(total)]))
    # a time that does not increase is refused and changes nothing; a gap empties the window
    with pytest.raises(ValueError, match="must increase"):
        again.update(frames[3], 2 * dt)
    assert len(again.intervals) == 2
    late = again.update(frames[3], 2 * dt + again.max_gap_seconds + 1.0)
    assert late.interval_mm is None and late.total_mm is None and again.intervals == [] and again.total() is None
    assert late.rate.cpu().numpy().tobytes() == rates[3].tobytes()
    resumed = again.update(frames[3], 2 * dt + again.max_gap_seconds + 1.0 + dt)
    assert resumed.seconds == dt and len(again.intervals) == 1
    assert _same(resumed.total_mm.cpu().numpy(), resumed.interval_mm.cpu().numpy())

    # without motion the interval shows one deposit per scan and a dip between; along the motion the path is filled
    still = rg.RainAccumulator(motion=None)
    assert still.steps == 1
    first_rate = still.update(frames[0], 0.0).rate.cpu().numpy()
    none_frame = still.update(frames[1], dt)
    assert none_frame.motion is None
    none = none_frame.interval_mm.cpu().numpy()
    zero, zero_lat = sc.one_node((0.0, 0.0))
    want = ao.accumulate(first_rate[None], none_frame.rate.cpu().numpy()[None], zero, zero_lat, dt / 3600.0, 1).out[0]
    assert np.array_equal(_bits(none), _bits(want))
    path = sc.centroid_path(0, 1)
    start, mid, end = path[0], path[len(path) // 2], path[-1]
    assert start == (18, 40) and end == (21, 38) and mid not in (start, end)
    assert none[mid] < 0.5 * none[start] and none[mid] < 0.5 * none[end]
    clear = rg.RainAccumulator(**sc.FRAME_ESTIMATE)
    clear.update(frames[0], 0.0)
    auto = clear.update(frames[1], dt).interval_mm.cpu().numpy()
    assert all(auto[p] > 0.0 for p in path), [float(auto[p]) for p in path]
    assert auto[mid] > none[mid]
    whole = sc.centroid_path(0, 3)
    for t in (2, 3):
        last = clear.update(frames[t], t * dt)
    total = last.total_mm.cpu().numpy()
    assert len(whole) > len(path) and all(total[p] > 0.0 for p in whole)
    torch.cuda.synchronize()
