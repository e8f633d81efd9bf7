"""The nowcast kernels (csrc/rg_motion.hip, rg_accumulate.hip, rg_verify.hip, rg_convection.hip) where a launch-geometry
constant is exceeded, against the restatements of their families as they stand.  Scenes: tests/nowcast_scale_scenes.py;
tests/test_nowcast_scale_scenes.py proves on the CPU that each one reaches the path named here.

``layer_split``   40 000 layers: the second launch of ``rg_fss_sums_i32``, whose ``layer0`` is 32768;
``layer_limit``   65535 planes of 1 x 3: ``gridDim.y`` of ``contingency_kernel`` and ``sat_columns_kernel`` at its limit, the
                  sums in launches of 32768 and 32767 layers;
``four_trips``    1024 x 800: every workgroup of ``contingency_kernel`` and ``fss_sums_kernel`` makes three full trips of its
                  grid-stride loop and the first 128 a fourth;
``tall`` / ``wide``   8750 unrolled trips of the column pass and a remainder of 3; 1094 trips of the row pass, the last cut, the
                  carry beyond 2^16;
``plane_limit``   65535 planes of 2 x 3 through the echo table, the background, the centres and the area;
``wrap_row``      3 000 000 pixels in one row: the 64-bit prefix of the echo table passes 2^63 and wraps at 2^64 inside the row,
                  and every window sum comes out exact all the same;
``group_split``   262 140, 262 143 and 262 150 planes through ``rg_accumulate_advected_f32``: 65535 groups in one launch, with a
                  remainder, and 65537 groups -- a second launch that starts at plane 262 140 -- with a remainder;
``many_pairs``    4099 pairs: the pair of ``block_match_kernel`` from ``blockIdx.x / (nby * nbx)`` up to 4098, and the plane loop
                  of ``advect_kernel`` over 4099 planes.

Every comparison is exact: integers equal, floats bit for bit (NaN matched as NaN where the restatement is NumPy's and a NaN's
payload is not part of the contract).  The one place where the family's contract itself is wider -- q within one unit of
NumPy's at a rounding tie of ``exp10`` -- is treated as tests/test_gpu_convection.py treats it: the next stage is held EQUAL to
the restatement fed the device's q.  The raw C ABI writes between canaries; the public functions run wherever they take the
shape."""
import ctypes

import numpy as np
import pytest

import convection_oracle as co
import convection_scenes as cvs
import nowcast_scale_scenes as ns
import test_gpu_convection as family_convection
import verification_oracle as vo

pytestmark = pytest.mark.gpu
CANARY = 64                       # elements before and after every output
_PATTERN = {"uint8": 0xA5, "int16": -21555, "int32": -1234567, "int64": -1234567890123, "float32": -12345.5}


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


def _intact(env, buf, n):
    """The canaries on either side of the ``n`` elements, read back alone."""
    edge = env["torch"].cat([buf[:CANARY], buf[CANARY + n:]]).cpu().numpy()
    return len(edge) == 2 * CANARY and bool((edge == edge.dtype.type(_PATTERN[str(edge.dtype)])).all())


def _dev(env, a):
    return None if a is None else env["torch"].from_numpy(np.array(a)).to(env["dev"])     # a copy: the scenes are read-only


def _c(ctype, values):
    return (ctype * max(len(values), 1))(*values)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _periodic(env, base_t, count):
    """``base_t[p % PERIOD]`` for ``p`` below ``count``, gathered on the device."""
    torch = env["torch"]
    return base_t[torch.arange(count, device=env["dev"]) % ns.PERIOD].contiguous()


# ---- verification --------------------------------------------------------------------------------------------------------------
def _verification_raw(env, s):
    """One pass through the four entry points between canaries, the fraction at the smallest and at the largest scale;
    ``run()`` returns every output as an array and may be called again into the same buffers."""
    torch, nat, lib = env["torch"], env["native"], env["lib"]
    n, h, w = s.forecast.shape
    T, S = len(s.thresholds), len(s.scales)
    ends = (s.scales[0], s.scales[-1])
    f, o, m = _dev(env, s.forecast), _dev(env, s.observed), _dev(env, s.mask)
    thr, scales = _c(ctypes.c_float, s.thresholds), _c(ctypes.c_int32, s.scales)
    bufs = dict(counts=_guarded(env, (n, T, 3), "int64"), valid=_guarded(env, (n,), "int64"),
                sat_f=_guarded(env, (n, T, h, w), "int32"), sat_o=_guarded(env, (n, T, h, w), "int32"),
                sums=_guarded(env, (n, T, S, 3), "int64"), frac=_guarded(env, (2, n, T, h, w), "float32"))

    def run():
        view = {k: v[1] for k, v in bufs.items()}
        stream = nat.stream_ptr()
        with torch.cuda.device(env["dev"]):
            assert lib.rg_contingency_f32(nat.ptr(f), nat.ptr(o), nat.ptr(m), n, h, w, thr, T, nat.ptr(view["counts"]),
                                          nat.ptr(view["valid"]), stream) == 0
            assert lib.rg_exceedance_sat_i32(nat.ptr(f), nat.ptr(o), nat.ptr(m), n, h, w, thr, T, nat.ptr(view["sat_f"]), stream) == 0
            assert lib.rg_exceedance_sat_i32(nat.ptr(o), nat.ptr(f), nat.ptr(m), n, h, w, thr, T, nat.ptr(view["sat_o"]), stream) == 0
            assert lib.rg_fss_sums_i32(nat.ptr(view["sat_f"]), nat.ptr(view["sat_o"]), n * T, h, w, scales, S, nat.ptr(view["sums"]),
                                       stream) == 0
            for k, scale in enumerate(ends):
                assert lib.rg_box_fraction_f32(nat.ptr(view["sat_f"]), n * T, h, w, scale, nat.ptr(view["frac"][k]), stream) == 0
        torch.cuda.synchronize()
        for key, (buf, v) in bufs.items():
            assert _intact(env, buf, v.numel()), key
        return {k: v.cpu().numpy() for k, v in view.items()}

    return run, ends, (f, o, m)


@pytest.mark.parametrize("name", ns.VERIFICATION)
def test_verification_outputs_equal_the_restatement_and_repeat(env, name):
    s, want = ns.verification_scene(name), ns.verification_expected(name)
    n, h, w = s.forecast.shape
    run, ends, (f, o, m) = _verification_raw(env, s)
    got = run()
    print(f"{name}: {n} planes of {h} x {w}, {n * len(s.thresholds)} layers in launches of {ns.fss_launches(n * len(s.thresholds))}, "
          f"{ns.strips(h * w)} strips with trips {ns.strip_trips(h * w)}")
    assert np.array_equal(got["counts"], want.counts), f"{name}: {int((got['counts'] != want.counts).any(axis=(1, 2)).sum())} planes differ"
    assert np.array_equal(got["valid"], want.valid), name
    for key, table in (("sat_f", want.sat_f), ("sat_o", want.sat_o)):
        assert np.array_equal(got[key], table), f"{name}: {int((got[key] != table).sum())} entries of {key} differ"
    wrong = (got["sums"] != want.sums).any(axis=(2, 3)).reshape(-1)
    assert not wrong.any(), f"{name}: the sums of {int(wrong.sum())} layers differ, the first at layer {int(np.flatnonzero(wrong)[0])}"
    for k, scale in enumerate(ends):
        assert np.array_equal(_bits(got["frac"][k]), _bits(vo.box_fraction(want.sat_f, scale))), (name, scale)
    assert f.cpu().numpy().tobytes() == s.forecast.tobytes() and o.cpu().numpy().tobytes() == s.observed.tobytes()
    assert m is None or m.cpu().numpy().tobytes() == s.mask.tobytes()
    # a second call into the same buffers: the same bytes, so every launch clears and adds into its own layers only
    again = run()
    for key in got:
        assert again[key].tobytes() == got[key].tobytes(), (name, key)


@pytest.mark.parametrize("name", ("layer_split", "layer_limit"))
def test_the_public_functions_take_tens_of_thousands_of_layers(env, name):
    rg, torch = env["rg"], env["torch"]
    s, want = ns.verification_scene(name), ns.verification_expected(name)
    f, o, m = _dev(env, s.forecast), _dev(env, s.observed), _dev(env, s.mask)
    table = rg.contingency_device(f, o, s.thresholds, m)
    for k, member in enumerate((table.hits, table.false_alarms, table.misses)):
        assert member.dtype == torch.int64 and np.array_equal(member.cpu().numpy(), want.counts[..., k]), (name, k)
    assert np.array_equal(table.valid.cpu().numpy(), want.valid)
    assert np.array_equal(table.correct_negatives.cpu().numpy(), want.valid[:, None] - want.counts.sum(axis=-1))
    sums = rg.fss_device(f, o, s.thresholds, s.scales, m)
    assert np.array_equal(sums.sums.cpu().numpy(), want.sums) and np.array_equal(sums.observed.cpu().numpy(), want.sat_o[:, :, -1, -1])
    assert np.array_equal(sums.fss(), vo.fss(want.sums), equal_nan=True)


# ---- convection ----------------------------------------------------------------------------------------------------------------
def test_plane_limit_every_stage_equals_the_restatement_fed_the_stage_before(env):
    """tests/test_gpu_convection.py's chain, through its own staged run between canaries, on 65535 planes."""
    rg = env["rg"]
    s, want = ns.convection_scene("plane_limit"), ns.plane_limit_expected()
    run, (f, m) = family_convection._raw(env, s)
    got = run()
    assert int(np.abs(got["q"] - want.q).max()) <= 1
    assert np.array_equal(got["flag"], want.echo.astype(np.int32)) and np.array_equal(got["q"] > 0, want.echo)
    S, N, _ = co.background(s.dbz, s.hw, s.mask, s.min_dbz, q=got["q"])
    assert np.array_equal(got["S"], S), f"{int((got['S'] != S).any(axis=(1, 2)).sum())} planes of S differ"
    assert np.array_equal(got["N"], N) and np.array_equal(N, want.N)
    assert family_convection._within_one_step(got["bkg"], co.background_from_sums(got["S"], got["N"]))
    centres = co.centres(s.dbz, got["bkg"], s.edges, s.mask, s.min_dbz, s.intense, s.peak)
    assert np.array_equal(got["centres"], centres), f"{int((got['centres'] != centres).any(axis=(1, 2)).sum())} planes of centres differ"
    classes = co.area(got["centres"], s.dbz, s.footprints, s.mask, s.min_dbz)
    assert np.array_equal(got["classes"], classes), f"{int((got['classes'] != classes).any(axis=(1, 2)).sum())} planes of classes differ"
    assert got["centres"][-1].tobytes() == centres[-1].tobytes() and (got["classes"] == 2).any() and (got["classes"] == 1).any()
    assert f.cpu().numpy().tobytes() == s.dbz.tobytes() and m.cpu().numpy().tobytes() == s.mask.tobytes()
    # the public classification call returns the bits of the staged calls
    parts = rg.convective_stratiform_device(f, dx=cvs.DX, dy=cvs.DY, mask=m, return_parts=True)
    assert parts.classes.cpu().numpy().tobytes() == got["classes"].tobytes()
    assert parts.background.cpu().numpy().tobytes() == got["bkg"].tobytes()
    assert parts.centres.cpu().numpy().tobytes() == got["centres"].tobytes()


@pytest.mark.parametrize("name", ns.WRAP_ROWS)
def test_wrap_row_window_sums_are_exact_across_the_wrap_of_the_prefix(env, name):
    torch, nat, lib = env["torch"], env["native"], env["lib"]
    s = ns.convection_scene(name)
    shape = n, h, w = s.dbz.shape
    f = _dev(env, s.dbz)
    table_bytes = int(lib.rg_echo_table_bytes(n, h, w))
    assert table_bytes == (w + 1) * 16
    bufs = dict(table=_guarded(env, (table_bytes,), "uint8"), q=_guarded(env, shape, "int64"), flag=_guarded(env, shape, "int32"),
                S=_guarded(env, shape, "int64"), N=_guarded(env, shape, "int32"), bkg=_guarded(env, shape, "float32"))
    v = {k: b[1] for k, b in bufs.items()}
    stream = nat.stream_ptr()
    with torch.cuda.device(env["dev"]):
        assert lib.rg_echo_table_f32(nat.ptr(f), None, n, h, w, s.min_dbz, nat.ptr(v["table"]), table_bytes, stream) == 0
        assert lib.rg_disk_background(nat.ptr(v["table"]), n, h, w, _c(ctypes.c_int32, [0]), 0, nat.ptr(v["q"]), nat.ptr(v["flag"]), None,
                                      stream) == 0
        assert lib.rg_disk_background(nat.ptr(v["table"]), n, h, w, _c(ctypes.c_int32, s.hw), len(s.hw) - 1, nat.ptr(v["S"]),
                                      nat.ptr(v["N"]), nat.ptr(v["bkg"]), stream) == 0
    torch.cuda.synchronize()
    for key, (buf, view) in bufs.items():
        assert _intact(env, buf, view.numel()), key
    got = {k: view.cpu().numpy() for k, view in v.items() if k != "table"}
    prefix_end = int(v["table"][-16:].cpu().numpy().view(np.uint64)[0])      # the last entry's prefix of q: the row's total mod 2^64
    q = co.quantize(s.dbz, s.mask, s.min_dbz)
    total = sum(q.ravel().tolist())
    print(f"{name}: the row's q sums to {total / 2 ** 64:.4f} x 2^64; the table ends at {prefix_end}")
    if name == "wrap_row_uniform":
        want = ns.wrap_expected(name)                                          # 10^8 is exact: NumPy's q is the device's
        assert (got["q"] == ns.WRAP_Q).all() and total > 2 ** 64 and prefix_end == total - 2 ** 64
        assert np.array_equal(got["S"], got["N"].astype(np.int64) * ns.WRAP_Q), "S != N * q somewhere"
        assert np.array_equal(got["N"][0, 0], ns.wrap_window()) and (got["bkg"] == np.float32(80.0)).all()
    else:
        assert int(np.abs(got["q"] - q).max()) <= 1                            # the family's contract; S is held to the device's q
        want = ns.wrap_background(name, q=got["q"])
        assert prefix_end == sum(got["q"].ravel().tolist()) % 2 ** 64
    assert np.array_equal(got["flag"], (want[0] > 0).astype(np.int32))
    wrong = got["S"] != want[1]
    assert not wrong.any(), f"{name}: {int(wrong.sum())} sums differ, the first at column {int(np.flatnonzero(wrong.ravel())[0])}"
    assert np.array_equal(got["N"], want[2])
    off = _bits(got["bkg"]) != _bits(want[3])
    print(f"{name}: {int(off.sum())} background values differ from the restatement's bits")
    assert not off.any()
    assert f.cpu().numpy().tobytes() == s.dbz.tobytes()


# ---- accumulation --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ns.GROUP_SPLIT_METHODS)
@pytest.mark.parametrize("planes", ns.GROUP_SPLIT_PLANES)
def test_group_split_equals_the_periodic_restatement(env, planes, method):
    """Plane ``p`` holds base plane ``p % 61`` and must come out as the restatement of that base plane: compared on the
    device, ``out`` as bits."""
    torch, nat, rg = env["torch"], env["native"], env["rg"]
    s, want = ns.group_split_scene(method), ns.group_split_expected(method)
    h, w = ns.GROUP_SPLIT_SHAPE
    runs, rest = ns.accumulation_runs(planes)
    prev_t, next_t = _periodic(env, _dev(env, s.prev), planes), _periodic(env, _dev(env, s.next), planes)
    want_out = _periodic(env, _dev(env, _bits(want.out).view(np.int32)), planes)
    want_steps = _periodic(env, _dev(env, want.steps), planes)
    field_t = _dev(env, s.motion)
    bo, out = _guarded(env, (planes, h, w), "float32")
    bs, steps = _guarded(env, (planes, h, w), "uint8")
    with torch.cuda.device(env["dev"]):
        status = env["lib"].rg_accumulate_advected_f32(nat.ptr(prev_t), nat.ptr(next_t), planes, h, w, nat.ptr(field_t),
                                                       nat.MotionLattice(*s.lattice), s.hours, s.n_steps, s.substeps,
                                                       env["motion"].ADVECT_METHODS[method], s.min_steps, s.fill, nat.ptr(out),
                                                       nat.ptr(steps), nat.stream_ptr())
    print(f"group_split {planes} planes, {method}: launches of {runs} groups and a remainder of {rest} planes; status {status}"
          + ("" if status == 0 else f": {env['lib'].rg_last_error().decode()}"))
    assert status == nat.RG_OK
    torch.cuda.synchronize()
    assert _intact(env, bo, planes * h * w) and _intact(env, bs, planes * h * w)
    wrong = (out.view(torch.int32) != want_out).view(planes, -1).any(dim=1)
    assert not bool(wrong.any()), f"{int(wrong.sum())} planes of out differ, the first is plane {int(torch.nonzero(wrong)[0])}"
    assert torch.equal(out.view(torch.int32), want_out) and torch.equal(steps, want_steps)
    # the public function: the same bits
    depth, count = rg.accumulate_device(prev_t, next_t, field_t, s.hours, steps=s.n_steps, lattice=s.lattice, method=method,
                                        substeps=s.substeps, min_steps=s.min_steps, fill_value=s.fill, return_steps=True)
    assert torch.equal(depth.view(torch.int32), want_out) and torch.equal(count, want_steps)


# ---- motion --------------------------------------------------------------------------------------------------------------------
def test_many_pairs_block_match_equals_the_periodic_restatement(env):
    torch, nat, rg = env["torch"], env["native"], env["rg"]
    prev, nxt = ns.many_pairs_levels()
    want = ns.many_pairs_match()
    n, (h, w) = ns.MANY_PAIRS, ns.PAIR_SHAPE
    nby, nbx = want.valid.shape[1:]
    prev_t, next_t = _periodic(env, _dev(env, prev), n), _periodic(env, _dev(env, nxt), n)
    bd, disp = _guarded(env, (n, nby, nbx, 2), "int16")
    bm, motion = _guarded(env, (n, nby, nbx, 2), "float32")
    bs, score = _guarded(env, (n, nby, nbx), "float32")
    with torch.cuda.device(env["dev"]):
        assert env["lib"].rg_block_match_u8(nat.ptr(prev_t), nat.ptr(next_t), n, h, w, ns.PAIR_B, ns.PAIR_S, ns.PAIR_R,
                                            ns.PAIR_B * ns.PAIR_B // 8, nat.ptr(disp), nat.ptr(motion), nat.ptr(score),
                                            nat.stream_ptr()) == 0
    torch.cuda.synchronize()
    for buf, per in ((bd, 2), (bm, 2), (bs, 1)):
        assert _intact(env, buf, n * nby * nbx * per)
    got_disp, got_motion, got_score = disp.cpu().numpy(), motion.cpu().numpy(), score.cpu().numpy()
    want_disp = ns.periodic(want.disp, n)
    want_motion, want_score = ns.periodic(want.motion.astype(np.float32), n), ns.periodic(want.score.astype(np.float32), n)
    wrong = (got_disp != want_disp).any(axis=(1, 2, 3))
    assert not wrong.any(), f"disp of {int(wrong.sum())} pairs differs, the first is pair {int(np.flatnonzero(wrong)[0])}"
    for what, got, expected in (("score", got_score, want_score), ("motion", got_motion, want_motion)):
        assert np.array_equal(np.isnan(got), np.isnan(expected)), f"{what}: NaN sets differ"
        live = ~np.isnan(expected)
        off = _bits(got)[live] != _bits(expected)[live]
        print(f"many_pairs {what}: {int(off.sum())} of {int(live.sum())} values differ from the restatement's bits")
        assert not off.any(), what
    assert np.isnan(got_score).any() and not np.isnan(got_score).all(axis=(1, 2)).any()
    # the public function on the levels themselves: the same grid
    grid = rg.estimate_motion_device(prev_t, next_t, block=ns.PAIR_B, stride=ns.PAIR_S, search=ns.PAIR_R)
    assert grid.disp.cpu().numpy().tobytes() == got_disp.tobytes() and grid.motion.cpu().numpy().tobytes() == got_motion.tobytes()
    assert grid.score.cpu().numpy().tobytes() == got_score.tobytes()


@pytest.mark.parametrize("method", ns.ADVECT_METHODS)
def test_many_planes_advect_equals_the_periodic_restatement(env, method):
    torch, nat, rg = env["torch"], env["native"], env["rg"]
    planes, field, lat = ns.advect_base()
    n, (h, w), leads = ns.MANY_PAIRS, ns.PAIR_SHAPE, ns.ADVECT_LEADS
    src_t, field_t = _periodic(env, _dev(env, planes), n), _dev(env, field)
    want = _dev(env, _bits(ns.advect_expected(method)).view(np.int32))              # [leads, PERIOD, h, w] as bits
    want = torch.stack([_periodic(env, lead, n) for lead in want])
    buf, out = _guarded(env, (len(leads), n, h, w), "float32")
    with torch.cuda.device(env["dev"]):
        assert env["lib"].rg_advect_f32(nat.ptr(src_t), n, h, w, nat.ptr(field_t), nat.MotionLattice(*lat), _c(ctypes.c_double, leads),
                                        len(leads), ns.ADVECT_SUBSTEPS, env["motion"].ADVECT_METHODS[method], ns.ADVECT_FILL,
                                        nat.ptr(out), nat.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert _intact(env, buf, len(leads) * n * h * w)
    wrong = (out.view(torch.int32) != want).view(len(leads), n, -1).any(dim=2)
    assert not bool(wrong.any()), f"{int(wrong.sum())} advected planes differ, the first is {torch.nonzero(wrong)[0].tolist()}"
    assert torch.equal(out.view(torch.int32), want)
    there = rg.advect_device(src_t, field_t, leads, lattice=lat, method=method, substeps=ns.ADVECT_SUBSTEPS, fill_value=ns.ADVECT_FILL)
    assert torch.equal(there.view(torch.int32), want)
