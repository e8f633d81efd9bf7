"""Nowcast verification on the GPU (csrc/rg_verify.hip, radar_processor_amd/verification.py) against the NumPy restatement of
tests/verification_oracle.py on the scenes of tests/verification_scenes.py, through the raw C ABI between canaries and through
the public functions.

Every count, table entry and sum is an integer and the fraction is one correctly rounded division, so nothing here has a
tolerance: the outputs are EQUAL to the restatement."""
import ctypes

import numpy as np
import pytest

import verification_oracle as vo
import verification_scenes as sc

pytestmark = pytest.mark.gpu
CANARY = 64                       # elements before and after every output
_PATTERN = {"int32": -1234567, "int64": -1234567890123, "float32": -12345.5}


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


def _dev(env, a):
    return None if a is None else env["torch"].from_numpy(np.array(a)).to(env["dev"])     # a copy: the scenes are read-only


def _c(ctype, values):
    return (ctype * len(values))(*values)


def _raw(env, s):
    """One pass through the four entry points between canaries: ``(counts, valid, sat_f, sat_o, sums, fractions)`` as arrays
    plus the buffers, for a second pass into the same memory."""
    torch, nat, lib = env["torch"], env["native"], env["lib"]
    n, h, w = s.forecast.shape
    T, S = len(s.thresholds), len(s.scales)
    f, o, m = _dev(env, s.forecast), _dev(env, s.observed), _dev(env, s.mask)
    thr, scales = _c(ctypes.c_float, s.thresholds), _c(ctypes.c_int32, s.scales)
    bufs = dict(counts=_guarded(env, (n, T, 3), "int64"), valid=_guarded(env, (n,), "int64"),
                sat_f=_guarded(env, (n, T, h, w), "int32"), sat_o=_guarded(env, (n, T, h, w), "int32"),
                sums=_guarded(env, (n, T, S, 3), "int64"), frac=_guarded(env, (S, n, T, h, w), "float32"))

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
            for k, scale in enumerate(s.scales):
                assert lib.rg_box_fraction_f32(nat.ptr(view["sat_f"]), n * T, h, w, scale, nat.ptr(view["frac"][k]), stream) == 0
        torch.cuda.synchronize()
        for key, (buf, v) in bufs.items():
            assert _intact(buf, v.numel()), key
        return {k: v.cpu().numpy() for k, v in view.items()}

    return run, (f, o, m)


# ---- the raw C ABI against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.SCENES)
def test_every_output_equals_the_restatement(env, name):
    s, want = sc.scene(name), sc.expected(name)
    run, (f, o, m) = _raw(env, s)
    got = run()
    assert np.array_equal(got["counts"], want.counts), (name, got["counts"].tolist(), want.counts.tolist())
    assert np.array_equal(got["valid"], want.valid), name
    for key, table in (("sat_f", want.sat_f), ("sat_o", want.sat_o)):
        assert np.array_equal(got[key], table), f"{name}: {int((got[key] != table).sum())} entries of {key} differ"
    assert np.array_equal(got["sums"], want.sums), (name, got["sums"].tolist(), want.sums.tolist())
    for k, scale in enumerate(s.scales):
        frac = vo.box_fraction(want.sat_f, scale)
        assert np.array_equal(got["frac"][k].view(np.uint32), frac.view(np.uint32)), (name, scale)
    # inputs byte-unchanged
    assert f.cpu().numpy().tobytes() == s.forecast.tobytes() and o.cpu().numpy().tobytes() == s.observed.tobytes()
    assert m is None or m.cpu().numpy().tobytes() == s.mask.tobytes()
    # a second call into the same buffers: the same bytes, so the entry points clear what they sum into
    again = run()
    for key in got:
        assert again[key].tobytes() == got[key].tobytes(), (name, key)


def test_big_sums_is_the_closed_form(env):
    s = sc.scene("big_sums")
    closed = sc.sum_of_squared_areas(300, 300, 255)
    sums = env["rg"].fss_device(s.forecast, s.observed, s.thresholds, s.scales).sums.cpu().numpy()
    assert sums[0, 0, 0].tolist() == [closed, closed, 0] and closed > 2 ** 47


# ---- the public functions ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("rim", "rows", "line_v", "many"))
def test_public_functions_tensors_arrays_and_every_plane_alone(env, name):
    rg = env["rg"]
    s, want = sc.scene(name), sc.expected(name)
    f, o, m = _dev(env, s.forecast), _dev(env, s.observed), _dev(env, s.mask)
    table = rg.contingency_device(f, o, s.thresholds, m)
    for k, member in enumerate((table.hits, table.false_alarms, table.misses)):
        assert member.dtype == env["torch"].int64 and np.array_equal(member.cpu().numpy(), want.counts[..., k]), (name, k)
    negatives = want.valid[:, None] - want.counts.sum(axis=-1)
    assert np.array_equal(table.correct_negatives.cpu().numpy(), negatives) and np.array_equal(table.valid.cpu().numpy(), want.valid)
    sums = rg.fss_device(f, o, s.thresholds, s.scales, m)
    assert np.array_equal(sums.sums.cpu().numpy(), want.sums) and sums.pixels.tolist() == [s.forecast[0].size] * len(s.forecast)
    assert np.array_equal(sums.observed.cpu().numpy(), want.sat_o[:, :, -1, -1])
    assert np.array_equal(sums.fss(), vo.fss(want.sums), equal_nan=True)
    assert np.array_equal(rg.exceedance_sat_device(f, s.thresholds, o, m).cpu().numpy(), want.sat_f)
    # arrays in: the same result
    both = rg.verify_nowcast(s.forecast, s.observed, s.thresholds, s.scales, s.mask)
    assert np.array_equal(both.fss.sums.cpu().numpy(), want.sums) and np.array_equal(both.contingency.hits.cpu().numpy(), want.counts[..., 0])
    assert np.array_equal(both.contingency.valid.cpu().numpy(), want.valid)
    # every plane on its own equals its slice
    for p in range(len(s.forecast)):
        one = rg.verify_nowcast(f[p], s.observed[p], s.thresholds, s.scales, None if m is None else m[p])
        assert np.array_equal(one.fss.sums.cpu().numpy(), want.sums[p:p + 1]), (name, p)
        assert np.array_equal(one.contingency.misses.cpu().numpy(), want.counts[p:p + 1, :, 2]), (name, p)
        assert np.array_equal(rg.exceedance_sat_device(s.observed[p], s.thresholds, f[p], None if m is None else m[p]).cpu().numpy(),
                              want.sat_o[p:p + 1]), (name, p)
    got = rg.categorical_scores(table)
    ref = vo.scores(want.counts[..., 0], want.counts[..., 1], want.counts[..., 2], negatives)
    for key, v in ref.items():
        assert np.array_equal(got[key], v, equal_nan=True), (name, key)


def test_tables_and_sums_add_exactly_on_the_device(env):
    rg = env["rg"]
    a, b = sc.scene("rows"), sc.scene("rows")
    first = rg.verify_nowcast(a.forecast, a.observed, a.thresholds, a.scales, a.mask)
    second = rg.verify_nowcast(b.observed, b.forecast, b.thresholds, b.scales)              # the roles swapped, no mask
    total = first + second
    want_a, want_b = sc.expected("rows"), vo.contingency(b.observed, b.forecast, b.thresholds)
    assert np.array_equal(total.contingency.hits.cpu().numpy(), want_a.counts[..., 0] + want_b.counts[..., 0])
    assert np.array_equal(total.contingency.false_alarms.cpu().numpy(), want_a.counts[..., 1] + want_b.counts[..., 1])
    assert np.array_equal(total.contingency.valid.cpu().numpy(), want_a.valid + want_b.valid)
    assert np.array_equal(total.fss.sums.cpu().numpy(), want_a.sums + vo.fss_sums(b.observed, b.forecast, b.thresholds, b.scales))
    assert total.fss.pixels.tolist() == [2 * 45 * 150] * 3
    assert np.array_equal((first.fss + first.fss).fss(), first.fss.fss(), equal_nan=True)


def test_the_neighbourhood_fraction(env):
    rg = env["rg"]
    s = sc.scene("rows")
    hit = vo.exceedance(s.forecast, s.thresholds, None, s.mask)
    one = rg.neighbourhood_fraction_device(s.forecast, s.thresholds, 1, s.mask)
    assert one.dtype == env["torch"].float32 and tuple(one.shape) == hit.shape
    assert np.array_equal(one.cpu().numpy(), hit.astype(np.float32))                         # scale 1: the exceedance itself
    table = vo.sat(s.forecast, s.thresholds, None, s.mask)
    for scale in (2, 31, 255):
        got = rg.neighbourhood_fraction_device(_dev(env, s.forecast), s.thresholds, scale, _dev(env, s.mask)).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), vo.box_fraction(table, scale).view(np.uint32)), scale
    single = rg.neighbourhood_fraction_device(s.forecast[1], s.thresholds[2:3], 8).cpu().numpy()
    assert single.shape == (1, 1, 45, 150)
    assert np.array_equal(single, vo.box_fraction(vo.sat(s.forecast[1], s.thresholds[2:3]), 8))


# ---- the verifier --------------------------------------------------------------------------------------------------------------
def _oracle_totals(frames, results, which):
    """Per lead, the sum of oracle calls on the forecasts the verifier returned."""
    L, T, S = len(sc.SEQ_LEADS), len(sc.SEQ_THRESHOLDS), len(sc.SEQ_SCALES)
    counts, valid, sums = np.zeros((L, T, 3), np.int64), np.zeros(L, np.int64), np.zeros((L, T, S, 3), np.int64)
    verified = [0] * L
    for r in results:
        for li, lead in enumerate(sc.SEQ_LEADS):
            target = r.frame + lead
            if target >= len(frames):
                continue
            forecast = r.source if which == "persistence" else (None if r.forecasts is None else r.forecasts[li])
            if forecast is None:
                continue
            forecast = forecast.cpu().numpy()
            c = vo.contingency(forecast, frames[target], sc.SEQ_THRESHOLDS)
            counts[li] += c.counts[0]
            valid[li] += c.valid[0]
            sums[li] += vo.fss_sums(forecast, frames[target], sc.SEQ_THRESHOLDS, sc.SEQ_SCALES)[0]
            verified[li] += 1
    return counts, valid, sums, verified


def _check_totals(verifier, frames, results):
    for which in ("nowcast", "persistence"):
        counts, valid, sums, verified = _oracle_totals(frames, results, which)
        total = verifier.totals(which)
        assert np.array_equal(total.contingency.hits.cpu().numpy(), counts[..., 0]), which
        assert np.array_equal(total.contingency.false_alarms.cpu().numpy(), counts[..., 1]), which
        assert np.array_equal(total.contingency.misses.cpu().numpy(), counts[..., 2]), which
        assert np.array_equal(total.contingency.valid.cpu().numpy(), valid), which
        assert np.array_equal(total.fss.sums.cpu().numpy(), sums), which
        assert verifier.scores()[which]["verified"] == tuple(verified), which


def test_the_verifier_with_the_exact_motion(env):
    rg = env["rg"]
    frames = sc.blob_sequence()
    field = np.array([[sc.SEQ_MOTION]], dtype=np.float32)
    lattice = (0.0, 0.0, 1.0, 1.0, 1, 1)
    verifier = rg.NowcastVerifier(sc.SEQ_LEADS, sc.SEQ_THRESHOLDS, sc.SEQ_SCALES, motion=(field, lattice), method="nearest")
    results = [verifier.update(frame) for frame in frames]
    assert [r.verified for r in results] == [(), (1,), (1, 2), (1, 2, 3), (1, 2, 3), (1, 2, 3)]
    assert all(tuple(r.forecasts.shape) == (3,) + sc.SEQ_SHAPE for r in results)
    _check_totals(verifier, frames, results)
    scores = verifier.scores()
    assert scores["nowcast"]["verified"] == (5, 4, 3) == scores["persistence"]["verified"]
    sums = verifier.totals("nowcast").fss.sums.cpu().numpy()
    reached = slice(0, len(sc.SEQ_THRESHOLDS) - 1)
    assert not sums[..., 0].any() and (sums[:, reached, :, 1] > 0).all()                     # A == 0 wherever the blobs reach
    assert (scores["nowcast"]["fss"][:, reached] == 1.0).all() and np.isnan(scores["nowcast"]["fss"][:, -1]).all()
    assert (scores["nowcast"]["csi"][:, reached] == 1.0).all() and (scores["nowcast"]["far"][:, reached] == 0.0).all()
    assert (scores["persistence"]["fss"][:, reached, 0] < 1.0).all()                         # scale 1
    assert (scores["persistence"]["fss"][:, reached, 0] == 0.0).all()                        # rows apart: nothing overlaps
    assert (scores["nowcast"]["useful"] >= 0.5).all()
    verifier.reset()
    assert verifier.totals() is None and verifier.update(frames[0]).frame == 0


def test_the_verifier_with_estimated_motion(env):
    rg = env["rg"]
    frames = sc.blob_sequence()
    verifier = rg.NowcastVerifier(sc.SEQ_LEADS, sc.SEQ_THRESHOLDS, sc.SEQ_SCALES, motion="auto", block=16, stride=8, search=4,
                                  min_echo=8)
    results = [verifier.update(env["torch"].from_numpy(np.array(frame)).to(env["dev"])) for frame in frames]
    assert results[0].forecasts is None and results[0].motion is None and results[1].forecasts is not None
    assert [r.verified for r in results] == [(), (1,), (1, 2), (1, 2, 3), (1, 2, 3), (1, 2, 3)]
    _check_totals(verifier, frames, results)
    assert verifier.scores()["nowcast"]["verified"] == (4, 3, 2) and verifier.scores()["persistence"]["verified"] == (5, 4, 3)
    # zero motion: the nowcast is persistence
    still = rg.NowcastVerifier(sc.SEQ_LEADS, sc.SEQ_THRESHOLDS, sc.SEQ_SCALES, motion=None)
    for frame in frames:
        still.update(frame)
    assert np.array_equal(still.totals("nowcast").fss.sums.cpu().numpy(), still.totals("persistence").fss.sums.cpu().numpy())
    assert np.array_equal(still.totals("persistence").fss.sums.cpu().numpy(), verifier.totals("persistence").fss.sums.cpu().numpy())
