"""The chain split -> label -> regions -> edges -> apply captured into a graph on inputs A and replayed on inputs B, over dirtied
outputs and workspaces, through the raw C ABI -- what tests/test_gpu_phase_replay.py does for include/radargrid_phase.h, for the
entry points of include/radargrid_velocity.h.  ``CHAINED`` names every function of ``_native.VELOCITY_SIGNATURES`` that takes a
stream; the first test (CPU) holds that list complete.

The chain is linear, one stream, no parallel branches.  The host merge cannot run inside a graph, so the fold table is an input
like the others (the restatement's, padded to one length).  The replay gives B's result only if every launch went to the given
stream, the edge table and its totals were cleared by the graph itself, and nothing was read on the host or baked into a launch
argument from device data (the region count is device data: B's is another)."""
import ctypes

import numpy as np
import pytest

from radar_processor_amd import _native

import velocity_oracle as vo
import velocity_scenes as vs

CHAINED = ("rg_velocity_split_f32", "rg_velocity_regions_i32", "rg_region_edges_f32", "rg_velocity_apply_folds_f32")
S, R, G, B = 2, 36, 65, 3
NYQUIST = (10.0, 8.0)
MAX_REGIONS, MAX_EDGES = 64, 192          # more than either scene has: the table's size is a launch argument
FLT_MAX = float(np.finfo(np.float32).max)


def test_every_velocity_entry_point_that_takes_a_stream_is_in_the_chain():
    taking = {name for name, (_, argtypes) in _native.VELOCITY_SIGNATURES.items() if len(argtypes) > 1 and argtypes[-1] is ctypes.c_void_p}
    assert taking == set(CHAINED) and len(CHAINED) == len(set(CHAINED)) == 4
    import inspect
    import sys
    source = inspect.getsource(sys.modules[__name__].test_chain_captured_on_a_replays_on_b_and_on_dirtied_workspaces)
    assert all(f"lib.{name}(" in source for name in CHAINED)


def scene(which):
    """A: two wind sweeps, the second with holes.  B: the same shapes and Nyquist velocities over other rays: another wind, other
    holes, a mask."""
    if which == "A":
        vel = np.stack([vs.wind(R, G, NYQUIST[0], B, 22.0).vel, vs.wind(R, G, NYQUIST[1], B, 19.0, holes=0.10, seed=0).vel])
        mask = np.zeros((S, R, G), np.uint8)
    else:
        vel = np.stack([vs.wind(R, G, NYQUIST[0], B, 27.0, holes=0.05, seed=4).vel[::-1], np.roll(vs.wind(R, G, NYQUIST[1], B, 12.0).vel, 9, axis=0)])
        mask = (np.random.default_rng(8).random((S, R, G)) < 0.04).astype(np.uint8) * np.uint8(3)
    ref = vo.dealias(vel, NYQUIST, B, mask, True)
    lut = np.zeros(MAX_REGIONS, np.int32)
    lut[:ref.n_regions] = ref.lut
    return dict(vel=np.ascontiguousarray(vel), mask=mask, lut=lut), ref


_CACHE = {}


def cached(which):
    if which not in _CACHE:
        _CACHE[which] = scene(which)
    return _CACHE[which]


def test_the_two_scenes_differ_everywhere_that_matters():
    (_, a), (_, b) = cached("A"), cached("B")
    assert a.n_regions != b.n_regions and max(a.n_regions, b.n_regions) <= MAX_REGIONS
    assert len(a.edges) != len(b.edges) and max(len(a.edges), len(b.edges)) <= MAX_EDGES
    for x, y in ((a.regions, b.regions), (a.folds, b.folds), (a.velocity, b.velocity)):
        assert x.shape == y.shape == (S, R, G) and not np.array_equal(vo.bits(x), vo.bits(y))
    assert np.abs(a.folds).max() >= 1 and np.abs(b.folds).max() >= 1


@pytest.mark.gpu
def test_chain_captured_on_a_replays_on_b_and_on_dirtied_workspaces():
    import torch
    import radar_processor_amd as rg
    lib = rg.load_library()
    dev = torch.device("cuda", 0)
    P = _native.ptr
    t = {key: torch.empty(value.shape, dtype=getattr(torch, str(value.dtype)), device=dev) for key, value in cached("A")[0].items()}
    label_bytes = int(lib.rg_components_workspace_bytes(S * B, R, G))
    edge_bytes = int(lib.rg_region_edges_workspace_bytes(MAX_EDGES))
    assert label_bytes >= 0 and edge_bytes == 20 * 512
    out = dict(split=torch.empty((S, B, R, G), dtype=torch.float32, device=dev),
               labels=torch.empty((S * B, R, G), dtype=torch.int32, device=dev),
               cell_ptr=torch.empty(S * B + 1, dtype=torch.int32, device=dev),
               label_ws=torch.empty(max(label_bytes, 16) // 4, dtype=torch.int32, device=dev),
               regions=torch.empty((S, R, G), dtype=torch.int32, device=dev),
               pair_ids=torch.empty((MAX_EDGES, 2), dtype=torch.int32, device=dev),
               pair_count=torch.empty(MAX_EDGES, dtype=torch.int32, device=dev),
               pair_sum=torch.empty(MAX_EDGES, dtype=torch.int64, device=dev),
               totals=torch.empty(2, dtype=torch.int32, device=dev),
               edge_ws=torch.empty(edge_bytes // 8, dtype=torch.int64, device=dev),
               velocity=torch.empty((S, R, G), dtype=torch.float32, device=dev),
               folds=torch.empty((S, R, G), dtype=torch.int32, device=dev))
    nyq = (ctypes.c_double * S)(*NYQUIST)

    def load(which):
        for key, value in cached(which)[0].items():
            t[key].copy_(torch.from_numpy(np.array(value)))

    def dirty():
        for buf in out.values():
            buf.fill_(-12345.5 if buf.dtype == torch.float32 else 0x5A5A5A5A if buf.dtype == torch.int32 else 0x5A5A5A5A5A5A5A5A)

    def enqueue(stream):
        return [lib.rg_velocity_split_f32(P(t["vel"]), P(t["mask"]), S, R, G, nyq, B, P(out["split"]), stream),
                lib.rg_label_components_f32(P(out["split"]), 0, S * B, R, G, -FLT_MAX, float("inf"), 4, 1, P(out["labels"]),
                                            P(out["cell_ptr"]), P(out["label_ws"]), label_bytes, stream),
                lib.rg_velocity_regions_i32(P(out["labels"]), P(out["cell_ptr"]), S, R, G, B, P(out["regions"]), stream),
                lib.rg_region_edges_f32(P(t["vel"]), P(out["regions"]), S, R, G, 1, MAX_EDGES, P(out["pair_ids"]), P(out["pair_count"]),
                                        P(out["pair_sum"]), P(out["totals"]), P(out["edge_ws"]), edge_bytes, stream),
                lib.rg_velocity_apply_folds_f32(P(t["vel"]), P(out["regions"]), P(t["lut"]), MAX_REGIONS, S, R, G, nyq,
                                                P(out["velocity"]), P(out["folds"]), stream)]

    def read():
        torch.cuda.synchronize()
        got = {key: out[key].cpu().numpy() for key in ("split", "cell_ptr", "regions", "totals", "velocity", "folds")}
        held = int(got["totals"][0])
        assert 0 <= held <= MAX_EDGES
        rows = np.concatenate([out["pair_ids"].cpu().numpy()[:held].astype(np.int64), out["pair_count"].cpu().numpy()[:held, None].astype(np.int64),
                               out["pair_sum"].cpu().numpy()[:held, None]], axis=1)
        got["edges"] = rows[np.lexsort((rows[:, 1], rows[:, 0]))]          # the order of the rows is unspecified: compare the set
        return got

    def check(got, which):
        inputs, ref = cached(which)
        want = vo.regions(inputs["vel"], NYQUIST, B, inputs["mask"], True)
        np.testing.assert_array_equal(vo.bits(got["split"]), vo.bits(vo.split(inputs["vel"], NYQUIST, B, inputs["mask"])), err_msg=which)
        np.testing.assert_array_equal(got["cell_ptr"], want.cell_ptr, err_msg=which)
        np.testing.assert_array_equal(got["regions"], ref.regions, err_msg=which)
        assert got["totals"].tolist() == [len(ref.edges), 0], which
        np.testing.assert_array_equal(got["edges"], ref.edges, err_msg=which)
        np.testing.assert_array_equal(got["folds"], ref.folds, err_msg=which)
        np.testing.assert_array_equal(vo.bits(got["velocity"]), vo.bits(ref.velocity), err_msg=which)

    # eagerly on A and on B: the module is loaded, and these are the results every replay has to equal
    eager = {}
    for which in ("A", "B"):
        load(which)
        dirty()
        assert enqueue(_native.stream_ptr()) == [0] * 5, lib.rg_last_error().decode()
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
    assert statuses == [0] * 5, lib.rg_last_error().decode()
    for step, which in enumerate(("B", "B", "A", "B")):
        load(which)
        if step != 1:
            dirty()                                                         # step 1: B's own results stand in the outputs
        graph.replay()
        got = read()
        check(got, which)
        for key in got:
            assert got[key].tobytes() == eager[which][key].tobytes(), f"replay {step} on {which}: {key} is not the eager call's"
