"""The texture and the classifier captured into a graph on inputs A and replayed on inputs B, over dirtied outputs, through the raw
C ABI -- what tests/test_gpu_shear_replay.py does for include/radargrid_shear.h, for the entry points of
include/radargrid_hydro.h.  ``CHAINED`` names every function of ``_native.HYDRO_SIGNATURES``; the first test (CPU) holds that list
complete.

The chain is linear, one stream, no parallel branches: the texture's sd is a variable of the classifier, and the condition
variable at that.  B has another field, another mask, another per-sweep row AND ANOTHER TABLE in the same device buffer: the replay
gives B's result only if every launch went to the given stream, the cells were read from the device at run time and not on the
host at capture, and every output byte is written by the kernels themselves.  What the header passes by value (weights, edges,
kinds, min_score) is the same for A and B."""
import ctypes

import numpy as np
import pytest

from radar_processor_amd import _native

import hydro_oracle as ho

CHAINED = ("rg_polar_texture_f32", "rg_fuzzy_classify_f32")
R, G, S = 6, 700, 3                          # two tiles per ray, the second one short
HALF_GATES, MIN_VALID = 3, 3
KINDS, EDGES, MIN_SCORE = (0, 0, 1), (1.0, 2.5), 0.2
WEIGHTS = np.array([[1.0, 0.5, 0.0], [0.75, 0.25, 0.0], [0.5, 0.0, 0.0]])
B_, C_, V_ = 3, 3, 3


def test_every_hydro_entry_point_takes_a_stream_and_is_in_the_chain():
    taking = {name for name, (_, argtypes) in _native.HYDRO_SIGNATURES.items() if len(argtypes) > 1 and argtypes[-1] is ctypes.c_void_p}
    assert taking == set(_native.HYDRO_SIGNATURES) == set(CHAINED) and len(CHAINED) == 2
    import inspect
    import sys
    source = inspect.getsource(sys.modules[__name__].test_chain_captured_on_a_replays_on_b_and_on_dirtied_outputs)
    assert all(f"lib.{name}(" in source for name in CHAINED)


def scene(which):
    """A: three plateaus of a noisy field.  B: the field reversed and shifted, other holes, a mask, another table."""
    rng = np.random.default_rng(41 if which == "A" else 42)
    level = np.array([5.0, 15.0, 25.0])[(np.arange(G) // 90) % 3]
    sigma = np.array([0.5, 1.7, 4.0])[(np.arange(G) // 30) % 3]           # textures in each of the three bins
    x = (level[None, :] + sigma[None, :] * rng.normal(0.0, 1.0, (R, G))).astype(np.float32)
    x[rng.random((R, G)) < (0.1 if which == "A" else 0.2)] = np.nan
    mask = np.zeros((R, G), np.uint8) if which == "A" else (rng.random((R, G)) < 0.1).astype(np.uint8)
    if which == "B":
        x = np.ascontiguousarray(x[:, ::-1] + np.float32(2.0))
    row = rng.uniform(-1.0, 1.0, (S, G)).astype(np.float32)
    row[:, ::13] = np.nan
    centre = np.array([5.0, 15.0, 25.0]) + (0.0 if which == "A" else 2.0)
    vert = np.zeros((B_, C_, V_, 4))
    for b in range(B_):
        for c in range(C_):
            half = 3.0 + b + (0.5 if which == "B" else 0.0)
            vert[b, c, 0] = (centre[c] - half - 2.0, centre[c] - half, centre[c] + half, centre[c] + half + 2.0)
            vert[b, c, 1] = (-np.inf, -np.inf, 2.0 + c, 4.0 + c + b)
            vert[b, c, 2] = (-1.5, -0.5 - 0.1 * c, 0.5, 0.9 if which == "A" else 1.2)
    spec = ho.Spec(KINDS, 1, 1, EDGES, ho.compile_cells(vert), WEIGHTS)
    tex = ho.texture(x, mask, HALF_GATES, MIN_VALID, 0)
    ref = ho.classify([x, tex.sd, row], 1 << 2, R // S, mask, spec, MIN_SCORE)
    return dict(x=x, mask=mask, row=row, cells=spec.cells), (tex, ref)


_CACHE = {}


def cached(which):
    if which not in _CACHE:
        _CACHE[which] = scene(which)
    return _CACHE[which]


def test_the_two_scenes_differ_everywhere_that_matters():
    (ia, (ta, a)), (ib, (tb, b)) = cached("A"), cached("B")
    assert ia["cells"].shape == ib["cells"].shape == (B_, C_, V_, 6) and not np.array_equal(ia["cells"], ib["cells"])
    assert not np.array_equal(ho.bits(ta.sd), ho.bits(tb.sd)) and not np.array_equal(ta.count, tb.count)
    assert not np.array_equal(a.cls, b.cls) and not np.array_equal(a.second, b.second)
    for tex, ref in ((ta, a), (tb, b)):
        assert set(np.unique(ref.cls).tolist()) == {0, 1, 2, 3} and 0.05 < (ref.cls == 0).mean() < 0.6
        assert np.isnan(tex.sd).any() and (~np.isnan(tex.sd)).mean() > 0.5
        with np.errstate(invalid="ignore"):
            assert all(((tex.sd >= lo) & (tex.sd < hi) & (ref.cls != 0)).any() for lo, hi in ((0.0, 1.0), (1.0, 2.5), (2.5, 99.0)))
    # B's inputs under A's table are something else again: the table is part of what the replay has to pick up
    mixed = ho.classify([ib["x"], tb.sd, ib["row"]], 1 << 2, R // S, ib["mask"],
                        ho.Spec(KINDS, 1, 1, EDGES, ia["cells"], WEIGHTS), MIN_SCORE)
    assert not np.array_equal(mixed.cls, b.cls)


@pytest.mark.gpu
def test_chain_captured_on_a_replays_on_b_and_on_dirtied_outputs():
    import torch
    import radar_processor_amd as rg
    lib = rg.load_library()
    dev = torch.device("cuda", 0)
    P = _native.ptr
    t = {key: torch.empty(value.shape, dtype=getattr(torch, str(value.dtype)), device=dev) for key, value in cached("A")[0].items()}
    out = dict(sd=torch.empty((R, G), dtype=torch.float32, device=dev), mean=torch.empty((R, G), dtype=torch.float32, device=dev),
               count=torch.empty((R, G), dtype=torch.int16, device=dev),           # the bits of uint16
               cls=torch.empty((R, G), dtype=torch.uint8, device=dev), score=torch.empty((R, G), dtype=torch.float32, device=dev),
               second=torch.empty((R, G), dtype=torch.uint8, device=dev))
    c_kinds = (ctypes.c_int32 * V_)(*KINDS)
    c_edges = (ctypes.c_double * len(EDGES))(*EDGES)
    c_weights = (ctypes.c_double * (C_ * V_))(*WEIGHTS.reshape(-1).tolist())

    def load(which):
        for key, value in cached(which)[0].items():
            t[key].copy_(torch.from_numpy(np.array(value)))

    def dirty():
        for buf in out.values():
            buf.fill_(-12345.5 if buf.dtype == torch.float32 else 0x5A)

    def enqueue(stream):
        c_vars = (ctypes.c_void_p * V_)(P(t["x"]), P(out["sd"]), P(t["row"]))
        return [lib.rg_polar_texture_f32(P(t["x"]), P(t["mask"]), R, G, HALF_GATES, MIN_VALID, 0, P(out["sd"]), P(out["mean"]),
                                         P(out["count"]), stream),
                lib.rg_fuzzy_classify_f32(c_vars, c_kinds, V_, 1 << 2, 1, R // S, P(t["mask"]), R, G, 1, c_edges, B_, P(t["cells"]), C_,
                                          c_weights, MIN_SCORE, P(out["cls"]), P(out["score"]), P(out["second"]), stream)]

    def read():
        torch.cuda.synchronize()
        return {key: buf.cpu().numpy() for key, buf in out.items()}

    def check(got, which):
        tex, ref = cached(which)[1]
        np.testing.assert_array_equal(ho.bits(got["sd"]), ho.bits(tex.sd), err_msg=f"{which}: sd")
        np.testing.assert_array_equal(ho.bits(got["mean"]), ho.bits(tex.mean), err_msg=f"{which}: mean")
        np.testing.assert_array_equal(got["count"].view(np.uint16), tex.count, err_msg=which)
        np.testing.assert_array_equal(got["cls"], ref.cls, err_msg=f"{which}: cls")
        np.testing.assert_array_equal(ho.bits(got["score"]), ho.bits(ref.score), err_msg=f"{which}: score")
        np.testing.assert_array_equal(got["second"], ref.second, err_msg=f"{which}: second")

    # eagerly on A and on B: the module is loaded, and these are the results every replay has to equal
    eager = {}
    for which in ("A", "B"):
        load(which)
        dirty()
        assert enqueue(_native.stream_ptr()) == [0] * 2, lib.rg_last_error().decode()
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
    assert statuses == [0] * 2, lib.rg_last_error().decode()
    for step, which in enumerate(("B", "B", "A", "B")):
        load(which)
        if step != 1:
            dirty()                                                         # step 1: B's own results stand in the outputs
        graph.replay()
        got = read()
        check(got, which)
        for key in got:
            assert got[key].tobytes() == eager[which][key].tobytes(), f"replay {step} on {which}: {key} is not the eager call's"
