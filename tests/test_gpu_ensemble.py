"""The probabilistic nowcasts on the device (csrc/rg_ensemble.hip) against the NumPy restatement of the header
(tests/ensemble_oracle.py) on the scenes of tests/ensemble_scenes.py, through the raw C ABI and through the wrappers of
radar_processor_amd/ensemble.py: ``counts``, ``members``, ``hist`` and ``valid`` EQUAL, ``prob`` and ``mean`` bit for bit
(compared as uint32, NaN at the same pixels).  Three checks rest on no oracle: zero shifts against ``advect_device``, integer
shifts under zero motion against plainly sliced indicator planes, and ``prob`` with and without the other outputs."""
import ctypes
import itertools

import numpy as np
import pytest

import ensemble_oracle as eo
import ensemble_scenes as es
import motion_oracle as mo
import test_ensemble_oracle as host

pytestmark = pytest.mark.gpu
ALL = ("prob", "counts", "members", "mean")
METHODS = {"nearest": 0, "bilinear": 1}


@pytest.fixture(scope="module")
def env():
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native
    lib = rg.load_library()
    return dict(torch=torch, rg=rg, native=_native, lib=lib, dev=torch.device("cuda", 0))


def _same_floats(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN at other pixels"
    live = ~np.isnan(want)
    assert np.array_equal(got.view(np.uint32)[live], want.view(np.uint32)[live]), \
        f"{what}: {int((got.view(np.uint32)[live] != want.view(np.uint32)[live]).sum())} values differ in their bits"


def _same(got, want, what):
    for name in ALL:
        if name in ("prob", "mean"):
            _same_floats(got[name], getattr(want, name), f"{what}: {name}")
        else:
            assert got[name].dtype == np.uint8 and np.array_equal(got[name], getattr(want, name)), f"{what}: {name}"


def _raw(env, s, want=ALL, shifts=None):
    """One call of rg_ensemble_exceedance_f32 on scene ``s``: name -> ndarray of the outputs in ``want``."""
    torch, nat, lib, dev = env["torch"], env["native"], env["lib"], env["dev"]
    h, w = s.src.shape
    L, T, M = len(s.leads), len(s.thresholds), s.n_members
    t = dict(src=torch.from_numpy(s.src.copy()).to(dev), motion=torch.from_numpy(s.motion.copy()).to(dev),
             shifts=torch.from_numpy(np.array(s.shifts if shifts is None else shifts, dtype=np.float64)).to(dev))
    shapes = dict(prob=((L, T, h, w), torch.float32), counts=((L, T, h, w), torch.uint8), members=((L, h, w), torch.uint8),
                  mean=((L, h, w), torch.float32))
    out = {name: torch.full(shapes[name][0], 77, dtype=shapes[name][1], device=dev) for name in want}
    status = lib.rg_ensemble_exceedance_f32(
        nat.ptr(t["src"]), h, w, nat.ptr(t["motion"]), nat.MotionLattice(*s.lattice), (ctypes.c_double * L)(*s.leads), L, s.substeps,
        METHODS[s.method], nat.ptr(t["shifts"]), M, (ctypes.c_float * T)(*[float(v) for v in s.thresholds]), T, s.min_members,
        *[nat.ptr(out.get(name)) for name in ALL], nat.stream_ptr())
    assert status == 0, lib.rg_last_error().decode()
    torch.cuda.synchronize()
    return {name: v.cpu().numpy() for name, v in out.items()}


def _wrapped(env, s, **kw):
    args = dict(lattice=tuple(s.lattice), method=s.method, substeps=s.substeps, min_members=s.min_members, want=ALL)
    args.update(kw)
    return env["rg"].ensemble_exceedance_device(s.src, s.motion, s.leads, s.shifts, s.thresholds, **args)


def _arrays(products):
    return {name: getattr(products, name).cpu().numpy() for name in ALL if getattr(products, name) is not None}


# ---- against the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(es.field_scenes()))
def test_raw_abi_equals_the_oracle(env, name):
    _same(_raw(env, es.field_scenes()[name]), es.expected(name), name)


@pytest.mark.parametrize("name", sorted(es.field_scenes()))
def test_wrapper_equals_the_oracle(env, name):
    s = es.field_scenes()[name]
    products = _wrapped(env, s)
    _same(_arrays(products), es.expected(name), name)
    assert products.n_members == s.n_members and products.leads == tuple(s.leads)
    assert np.array_equal(products.thresholds, s.thresholds) and products.prob.is_cuda


def test_a_nan_shift_makes_that_member_missing_and_nothing_else(env):
    """The caller's duty is a finite shift; a NaN one (possible in a tensor, which is not checked) costs one member at that
    lead -- for both sampling rules."""
    for method in ("nearest", "bilinear"):
        s = es.ties()._replace(method=method)
        shifts = np.array(s.shifts)
        shifts[1, 2, 0] = np.nan
        shifts[0, 4] = np.nan
        want = eo.exceedance(s.src, s.motion, s.lattice, s.leads, shifts, s.thresholds, s.substeps, method, s.min_members)
        fewer = eo.exceedance(s.src, s.motion, s.lattice, s.leads[1:], np.delete(shifts, 2, axis=1)[1:], s.thresholds, s.substeps,
                              method, s.min_members)
        assert np.array_equal(want.members[1], fewer.members[0]) and want.members.max() == s.n_members - 1
        _same(_raw(env, s, shifts=shifts), want, f"NaN shift, {method}")
        got = _wrapped(env, s._replace(shifts=env["torch"].from_numpy(shifts).to(env["dev"])))
        _same(_arrays(got), want, f"NaN shift in a tensor, {method}")


# ---- without the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rim-min1", "lattice", "caps"])
def test_zero_shifts_are_the_advection_m_times(env, name):
    s = es.field_scenes()[name]
    s = s._replace(shifts=np.zeros_like(s.shifts))
    M = s.n_members
    advected = env["rg"].advect_device(s.src, s.motion, s.leads, lattice=tuple(s.lattice), method=s.method,
                                       substeps=s.substeps).cpu().numpy()                        # [L, h, w], NaN outside
    got = _raw(env, s)
    with np.errstate(invalid="ignore"):
        exceeds = np.stack([advected >= t for t in s.thresholds], axis=1)
    assert np.array_equal(got["counts"], (M * exceeds).astype(np.uint8))
    assert np.array_equal(got["members"], np.where(np.isnan(advected), 0, M).astype(np.uint8))
    enough = M >= s.min_members
    assert enough
    _same_floats(got["mean"], advected, "the mean of M equal members")
    _same_floats(got["prob"], np.where(np.isnan(advected)[:, None], np.nan, exceeds.astype(np.float32)), "prob")


def test_integer_shifts_under_zero_motion_are_sliced_indicator_planes(env):
    base = es.rim(1)
    h, w = base.src.shape
    rng = np.random.default_rng(5)
    shifts = rng.integers(-7, 8, size=(2, 9, 2)).astype(np.float64)
    s = base._replace(motion=np.zeros_like(base.motion), shifts=shifts, leads=(1.0, 3.0), substeps=1)
    got = _raw(env, s)
    for l in range(2):
        counts = np.zeros((len(s.thresholds), h, w), np.int64)
        members = np.zeros((h, w), np.int64)
        for sy, sx in shifts[l].astype(int):                                  # the member at (y, x) is src[y - sy, x - sx]
            dst = (slice(max(sy, 0), min(h, h + sy)), slice(max(sx, 0), min(w, w + sx)))
            part = s.src[max(-sy, 0):min(h, h - sy), max(-sx, 0):min(w, w - sx)]
            members[dst] += ~np.isnan(part)
            with np.errstate(invalid="ignore"):
                for t, thr in enumerate(s.thresholds):
                    counts[t][dst] += part >= thr
        assert np.array_equal(got["counts"][l], counts) and np.array_equal(got["members"][l], members), l


def test_every_combination_of_null_outputs_gives_the_same_planes(env):
    s = es.rim(5)
    full = _raw(env, s)
    for r in range(1, 4):
        for want in itertools.combinations(ALL, r):
            got = _raw(env, s, want=want)
            assert sorted(got) == sorted(want)
            for name in want:
                assert got[name].tobytes() == full[name].tobytes(), (want, name)
    only = _arrays(_wrapped(env, s, want=("prob",)))
    assert list(only) == ["prob"] and only["prob"].tobytes() == full["prob"].tobytes()
    assert _wrapped(env, s, want="mean").prob is None


def test_no_leads_and_empty_planes(env):
    s = es.rim(1)
    none = env["rg"].ensemble_exceedance_device(s.src, s.motion, (), np.zeros((0, 5, 2)), s.thresholds, want=ALL)
    assert tuple(none.prob.shape) == (0, 3, 37, 53) and tuple(none.members.shape) == (0, 37, 53) and none.n_members == 5


# ---- refusals: the host-side list again, on addresses inside a real allocation, which stays untouched --------------------------------
def _rebase(args, positions, base):
    return tuple(base + a - host.P if k in positions and isinstance(a, int) and a else a for k, a in enumerate(args))


def test_every_refusal_returns_its_message_and_launches_nothing(env):
    torch, lib = env["torch"], env["lib"]
    arena = torch.full((80 * host.P,), 0x5A, dtype=torch.uint8, device=env["dev"])
    base = int(arena.data_ptr())
    for kw, message in host.EXCEEDANCE_REFUSALS:
        args = _rebase(host.exceedance_args(**kw), (0, 3, 9, 14, 15, 16, 17), base)
        assert lib.rg_ensemble_exceedance_f32(*args) == env["native"].RG_EINVAL, kw
        assert lib.rg_last_error().decode() == "rg_ensemble_exceedance_f32: " + message
    for kw, message in host.HISTOGRAM_REFUSALS:
        args = _rebase(host.histogram_args(**kw), (0, 1, 2, 3, 10, 11), base)
        assert lib.rg_ensemble_histogram_u8(*args) == env["native"].RG_EINVAL, kw
        assert lib.rg_last_error().decode() == "rg_ensemble_histogram_u8: " + message
    torch.cuda.synchronize()
    assert bool((arena == 0x5A).all())
    with pytest.raises(env["native"].NativeError, match="rg_ensemble_exceedance_f32: prob overlaps src"):
        plane = torch.zeros((4, 5), dtype=torch.float32, device=env["dev"])
        nat = env["native"]
        nat.check(lib.rg_ensemble_exceedance_f32(nat.ptr(plane), 4, 5, nat.ptr(arena), nat.MotionLattice(0, 0, 1, 1, 4, 5),
                                                 (ctypes.c_double * 1)(1.0), 1, 1, 0, nat.ptr(arena[4096:]), 1, (ctypes.c_float * 1)(1.0),
                                                 1, 1, nat.ptr(plane), None, None, None, nat.stream_ptr()), "rg_ensemble_exceedance_f32")


# ---- the histogram ---------------------------------------------------------------------------------------------------------------
def _raw_hist(env, s, garbage=-7):
    torch, nat, lib, dev = env["torch"], env["native"], env["lib"], env["dev"]
    n, T, h, w = s.counts.shape
    t = {k: torch.from_numpy(np.array(getattr(s, k))).to(dev) for k in ("counts", "members", "obs")}
    mask = None if s.mask is None else torch.from_numpy(np.array(s.mask)).to(dev)
    hist = torch.full((n, T, s.n_members + 1, 2), garbage, dtype=torch.int64, device=dev)         # the call clears them itself
    valid = torch.full((n,), garbage, dtype=torch.int64, device=dev)
    status = lib.rg_ensemble_histogram_u8(nat.ptr(t["counts"]), nat.ptr(t["members"]), nat.ptr(t["obs"]), nat.ptr(mask), n, h, w,
                                          s.n_members, (ctypes.c_float * T)(*[float(v) for v in s.thresholds]), T, nat.ptr(hist),
                                          nat.ptr(valid), nat.stream_ptr())
    assert status == 0, lib.rg_last_error().decode()
    torch.cuda.synchronize()
    return hist.cpu().numpy(), valid.cpu().numpy()


@pytest.mark.parametrize("name", sorted(es.HIST_SCENES))
def test_histogram_equals_the_oracle(env, name):
    s = es.HIST_SCENES[name]()
    hist, valid = _raw_hist(env, s)
    want_hist, want_valid = es.expected_hist(name)
    assert np.array_equal(valid, want_valid) and np.array_equal(hist, want_hist)
    assert (hist.sum(axis=(2, 3)) == valid[:, None]).all()
    if s.mask is not None:                                                    # without the mask: more pixels, the oracle's
        bare = s._replace(mask=None)
        got = _raw_hist(env, bare)
        want = eo.histogram(bare.counts, bare.members, bare.obs, None, bare.n_members, bare.thresholds)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[1].sum() > valid.sum()


def test_planted_pixels_are_left_out_and_nothing_else(env):
    s = es.planted()
    M = s.n_members
    hist, valid = _raw_hist(env, s)
    clean = s._replace(counts=np.minimum(s.counts, M), members=np.full_like(s.members, M), obs=np.nan_to_num(s.obs, nan=1.0), mask=None)
    _, all_valid = _raw_hist(env, clean)
    assert all_valid.tolist() == [19 * 67] * 3 and (all_valid - valid).tolist() == [7, 4, 3]


def test_histogram_through_the_wrappers_and_totals_of_two_scans(env):
    rg = env["rg"]
    s = es.lattice()._replace(min_members=1)
    obs = es.observed_for("lattice")
    mask = (np.random.default_rng(9).random(obs.shape) < 0.1).astype(np.uint8)
    products = _wrapped(env, s, want=("counts", "members"))
    want = es.expected("lattice")
    M = s.n_members
    assert (want.members < M).any() and (want.members == M).any()             # incomplete pixels are there to be left out
    tables = []
    for k, (o, m) in enumerate(((obs, mask), (obs[::-1].copy(), None))):
        table = rg.ensemble_histogram_device(products, o, m)
        want_hist, want_valid = eo.histogram(want.counts, want.members, o, m, M, s.thresholds)
        assert np.array_equal(table.hist.cpu().numpy(), want_hist) and np.array_equal(table.valid.cpu().numpy(), want_valid), k
        assert (table.hist.sum(dim=(2, 3)) == table.valid[:, None]).all() and table.n_members == M
        assert int(table.valid.sum()) < int(((want.members == M) & ~np.isnan(o)).sum()) + (0 if m is not None else 1)
        tables.append(table)
    total = tables[0] + tables[1]
    assert np.array_equal(total.hist.cpu().numpy(), tables[0].hist.cpu().numpy() + tables[1].hist.cpu().numpy())
    assert np.array_equal(total.valid.cpu().numpy(), tables[0].valid.cpu().numpy() + tables[1].valid.cpu().numpy())
    scores = rg.probability_scores(total)
    k = np.repeat(np.arange(M + 1), total.hist.cpu().numpy()[0, 1].sum(axis=1))
    o = np.concatenate([np.repeat([0, 1], row) for row in total.hist.cpu().numpy()[0, 1]])
    assert abs(scores["brier"][0, 1] - eo.brier_direct(k, o, M)) <= 1e-10 * eo.brier_direct(k, o, M)
    single = rg.ensemble_histogram_device(_wrapped(env, s._replace(leads=s.leads[:1], shifts=s.shifts[:1]), want=("counts", "members")),
                                          obs[0])
    assert np.array_equal(single.hist.cpu().numpy()[0], eo.histogram(want.counts[:1], want.members[:1], obs[:1], None, M,
                                                                     s.thresholds)[0][0])


# ---- the chain -----------------------------------------------------------------------------------------------------------------
def test_probabilistic_nowcast_is_its_four_stages(env):
    rg, torch = env["rg"], env["torch"]
    rng = np.random.default_rng(21)
    h, w = 96, 131
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")

    def frame(oy, ox):
        v = np.zeros((h, w))
        for cy, cx, s, a in ((30, 40, 9, 55), (60, 90, 14, 48), (75, 25, 6, 40)):
            v += a * np.exp(-((yy - cy - oy) ** 2 + (xx - cx - ox) ** 2) / (2.0 * s * s))
        return v.astype(np.float32)

    prev, nxt = frame(0, 0), frame(2, -3)
    nxt[rng.random((h, w)) < 0.01] = np.nan
    leads, thr, M = (1.0, 2.0, 4.0), (18.0, 35.0), 12
    kw = dict(par=(0.6, 0.5, 0.2), perp=(0.3, 0.5, 0.1), seed=4)
    products, grid = rg.probabilistic_nowcast_device(prev, nxt, leads, thr, M, block=32, stride=16, search=8, method="bilinear",
                                                     substeps=2, min_members=6, want=ALL, **kw)
    # the stages by hand
    by_hand = rg.fill_motion_device(rg.estimate_motion_device(prev, nxt, block=32, stride=16, search=8), 0.5)
    assert torch.equal(grid.motion, by_hand.motion)
    field = grid.motion.cpu().numpy()
    direction = field.astype(np.float64).mean(axis=(0, 1))
    assert abs(direction[0] - 2.0) < 0.5 and abs(direction[1] + 3.0) < 0.5    # the planted motion was found
    shifts = rg.motion_perturbations(M, leads, direction=direction, **kw)
    want = eo.exceedance(nxt, field, mo.Lattice(*grid.lattice), leads, shifts, np.array(thr, np.float32), 2, "bilinear", 6)
    _same(_arrays(products), want, "probabilistic_nowcast_device")
    assert 0.0 < np.nanmax(want.prob) <= 1.0 and ((want.prob > 0) & (want.prob < 1)).any()        # a spread, not a deterministic plane
    host_products, host_grid = rg.probabilistic_nowcast(prev, nxt, leads, thr, M, block=32, stride=16, search=8, method="bilinear",
                                                        substeps=2, min_members=6, want=ALL, **kw)
    assert all(isinstance(getattr(host_products, name), np.ndarray) for name in ALL) and isinstance(host_grid.motion, np.ndarray)
    _same({name: getattr(host_products, name) for name in ALL}, want, "probabilistic_nowcast")
