"""The chain ensemble -> histogram captured into a graph on inputs A and replayed on inputs B, with dirtied outputs, through the
raw C ABI -- what tests/test_gpu_graph_replay.py does for the entry points of include/radargrid_hip.h, for those of
include/radargrid_ensemble.h.  ``CHAINED`` names every function of ``_native.ENSEMBLE_SIGNATURES`` that takes a stream; the
first test (CPU) holds that list complete, as tests/test_stream_contract_host.py does for the other table.

The chain is linear, one stream, no parallel branches.  The replay gives B's result only if every launch and every clear went
to the given stream, nothing was read on the host or baked into a launch argument from device data (the shifts are device
data: B's are others), and ``hist`` and ``valid`` are cleared inside the call on every replay, not on the first one only."""
import ctypes

import numpy as np
import pytest

from radar_processor_amd import _native

import ensemble_oracle as eo
import ensemble_scenes as es

CHAINED = ("rg_ensemble_exceedance_f32", "rg_ensemble_histogram_u8")          # in the order of the chain below
ALL = ("prob", "counts", "members", "mean")
_GARBAGE = {"float32": -12345.5, "uint8": 0xA5, "int64": -1234567890123}


def test_every_ensemble_entry_point_that_takes_a_stream_is_in_the_chain():
    taking = {name for name, (_, argtypes) in _native.ENSEMBLE_SIGNATURES.items() if argtypes and argtypes[-1] is ctypes.c_void_p}
    assert taking == set(CHAINED) and len(CHAINED) == len(set(CHAINED)) == 2
    assert not any(name.endswith("_bytes") for name in CHAINED)
    import inspect
    import sys
    source = inspect.getsource(sys.modules[__name__].test_chain_captured_on_a_replays_on_b_and_on_dirtied_outputs)
    assert all(f"lib.{name}(" in source for name in CHAINED)


def scene(which):
    """A: the ``lattice`` scene.  B: the same shapes, leads and thresholds (host arguments: part of the graph) over another
    plane, another motion field and other shifts (device data: read at replay)."""
    a = es.lattice()
    if which == "A":
        return a, es.observed_for("lattice"), (np.random.default_rng(31).random((3,) + a.src.shape) < 0.08).astype(np.uint8)
    rng = np.random.default_rng(32)
    src = np.roll(a.src, (9, -13), axis=(0, 1)) * np.float32(0.9) + np.float32(3.0)
    b = a._replace(src=src, motion=(-a.motion[::-1]).copy(), shifts=rng.uniform(-5.0, 5.0, size=a.shifts.shape))
    obs = np.stack([np.roll(src, (k, 2 * k), axis=(0, 1)) for k in range(3)])
    return b, obs, (rng.random(obs.shape) < 0.15).astype(np.uint8) * np.uint8(3)


def expected(which):
    s, obs, mask = scene(which)
    fields = eo.exceedance(s.src, s.motion, s.lattice, s.leads, s.shifts, s.thresholds, s.substeps, s.method, s.min_members)
    return fields, eo.histogram(fields.counts, fields.members, obs, mask, s.n_members, s.thresholds)


def test_the_two_scenes_differ_everywhere_that_matters():
    (fa, (ha, va)), (fb, (hb, vb)) = expected("A"), expected("B")
    assert not np.array_equal(fa.counts, fb.counts) and not np.array_equal(fa.members, fb.members)
    assert not np.array_equal(ha, hb) and (va != vb).all() and va.min() > 100 and vb.min() > 100


@pytest.mark.gpu
def test_chain_captured_on_a_replays_on_b_and_on_dirtied_outputs():
    import torch
    import radar_processor_amd as rg
    lib = rg.load_library()
    dev = torch.device("cuda", 0)
    a = scene("A")[0]
    h, w = a.src.shape
    L, T, M = len(a.leads), len(a.thresholds), a.n_members
    leads, thr = (ctypes.c_double * L)(*a.leads), (ctypes.c_float * T)(*[float(v) for v in a.thresholds])
    t = dict(src=torch.empty((h, w), dtype=torch.float32, device=dev), motion=torch.empty(a.motion.shape, dtype=torch.float32, device=dev),
             shifts=torch.empty((L, M, 2), dtype=torch.float64, device=dev), obs=torch.empty((L, h, w), dtype=torch.float32, device=dev),
             mask=torch.empty((L, h, w), dtype=torch.uint8, device=dev))
    out = dict(prob=torch.empty((L, T, h, w), dtype=torch.float32, device=dev), counts=torch.empty((L, T, h, w), dtype=torch.uint8, device=dev),
               members=torch.empty((L, h, w), dtype=torch.uint8, device=dev), mean=torch.empty((L, h, w), dtype=torch.float32, device=dev),
               hist=torch.empty((L, T, M + 1, 2), dtype=torch.int64, device=dev), valid=torch.empty((L,), dtype=torch.int64, device=dev))
    P = _native.ptr

    def load(which):
        s, obs, mask = scene(which)
        for key, value in dict(src=s.src, motion=s.motion, shifts=s.shifts, obs=obs, mask=mask).items():
            t[key].copy_(torch.from_numpy(np.array(value)))

    def dirty():
        for key, buf in out.items():
            buf.fill_(_GARBAGE[str(buf.dtype).split(".")[-1]])

    def enqueue(stream):
        return [lib.rg_ensemble_exceedance_f32(P(t["src"]), h, w, P(t["motion"]), _native.MotionLattice(*a.lattice), leads, L, a.substeps,
                                               1, P(t["shifts"]), M, thr, T, a.min_members, P(out["prob"]), P(out["counts"]),
                                               P(out["members"]), P(out["mean"]), stream),
                lib.rg_ensemble_histogram_u8(P(out["counts"]), P(out["members"]), P(t["obs"]), P(t["mask"]), L, h, w, M, thr, T,
                                             P(out["hist"]), P(out["valid"]), stream)]

    def read():
        torch.cuda.synchronize()
        return {key: buf.cpu().numpy() for key, buf in out.items()}

    def check(got, which):
        fields, (hist, valid) = expected(which)
        assert np.array_equal(got["counts"], fields.counts) and np.array_equal(got["members"], fields.members), which
        assert np.array_equal(got["hist"], hist) and np.array_equal(got["valid"], valid), which
        for name in ("prob", "mean"):
            want = getattr(fields, name)
            assert np.array_equal(np.isnan(got[name]), np.isnan(want)), (which, name)
            live = ~np.isnan(want)
            assert np.array_equal(got[name].view(np.uint32)[live], want.view(np.uint32)[live]), (which, name)

    assert a.method == "bilinear"
    # eagerly on A and on B: the module is loaded, and these are the results every replay has to equal
    eager = {}
    for which in ("A", "B"):
        load(which)
        dirty()
        assert enqueue(_native.stream_ptr()) == [0, 0], lib.rg_last_error().decode()
        eager[which] = read()
        check(eager[which], which)
    # captured on A, on a side stream
    load("A")
    dirty()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        statuses = enqueue(_native.stream_ptr())
    assert statuses == [0, 0], lib.rg_last_error().decode()
    for step, which in enumerate(("B", "B", "A", "B")):
        load(which)
        if step != 1:
            dirty()                                                         # step 1: B's own results stand in the outputs
        graph.replay()
        got = read()
        check(got, which)
        for key in got:
            assert got[key].tobytes() == eager[which][key].tobytes(), f"replay {step} on {which}: {key} is not the eager call's"
