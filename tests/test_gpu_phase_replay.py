"""The chain unfold -> fit -> attenuation captured into a graph on inputs A and replayed on inputs B, with dirtied outputs,
through the raw C ABI -- what tests/test_gpu_ensemble_replay.py does for include/radargrid_ensemble.h, for the entry points of
include/radargrid_phase.h.  ``CHAINED`` names every function of ``_native.PHASE_SIGNATURES`` that takes a stream; the first test
(CPU) holds that list complete.

The chain is linear, one stream, no parallel branches.  The replay gives B's result only if every launch went to the given
stream and nothing was read on the host or baked into a launch argument from device data (the origin of a ray and the half-window
of a gate are device data: B's are others)."""
import ctypes

import numpy as np
import pytest

from radar_processor_amd import _native

import phase_oracle as po
import phase_scenes as ps

CHAINED = ("rg_phidp_unfold_f32", "rg_phidp_fit_f32", "rg_attenuation_phidp_f32")          # in the order of the chain below
WRAP, SPACING, EDGES, HALF, MIN_VALID, ALPHA, BETA, MAX_DPHI = 360.0, 240.0, (35.0, 48.0), (20, 10, 5), 6, 0.08, 0.02, 120.0
SCALE = 500.0 / (65536.0 * SPACING)
OUTPUTS = {"unfolded": "float32", "folds": "int32", "kdp": "float32", "phi_s": "float32", "count": "uint16", "dbz": "float32",
           "zdr": "float32", "pia": "float32", "dphi": "float32"}
_GARBAGE = {"float32": -12345.5, "int32": -1234567, "uint16": 0xA5A5}


def test_every_phase_entry_point_that_takes_a_stream_is_in_the_chain():
    taking = {name for name, (_, argtypes) in _native.PHASE_SIGNATURES.items() if argtypes and argtypes[-1] is ctypes.c_void_p}
    assert taking == set(CHAINED) and len(CHAINED) == len(set(CHAINED)) == 3
    import inspect
    import sys
    source = inspect.getsource(sys.modules[__name__].test_chain_captured_on_a_replays_on_b_and_on_dirtied_outputs)
    assert all(f"lib.{name}(" in source for name in CHAINED)


def scene(which):
    """A: the weather scene.  B: the same shapes and host arguments over other rays: reversed ray order, another offset, other
    holes, a mask, origins given for some rays."""
    w = ps.weather()
    R, G = w.phidp.shape
    if which == "A":
        return dict(phidp=w.phidp, mask=np.zeros((R, G), np.uint8), dbz=w.dbz, zdr=w.zdr, phi0=np.full(R, np.nan, np.float32))
    rng = np.random.default_rng(41)
    phidp = w.phidp[::-1].copy() + np.float32(25.0)
    phidp[phidp >= 180.0] -= np.float32(360.0)
    phidp[rng.random((R, G)) < 0.05] = np.nan
    phi0 = np.where(np.arange(R) % 2 == 0, np.float32(118.0), np.float32(np.nan)).astype(np.float32)
    return dict(phidp=phidp, mask=(rng.random((R, G)) < 0.1).astype(np.uint8) * np.uint8(2), dbz=np.roll(w.dbz, 17, axis=1) + np.float32(1.5),
                zdr=w.zdr[::-1] * np.float32(0.5), phi0=phi0)


def expected(which):
    s = scene(which)
    unfolded, folds = po.unfold(s["phidp"], s["mask"], WRAP)
    fit = po.fit(unfolded, SCALE, half_window=HALF, min_valid=MIN_VALID, dbz=s["dbz"], edges=EDGES)
    att = po.attenuation(fit.phi_s, s["dbz"], alpha=ALPHA, beta=BETA, max_dphi=MAX_DPHI, zdr=s["zdr"], phi0=s["phi0"])
    return dict(unfolded=unfolded, folds=folds, kdp=fit.kdp, phi_s=fit.phi_s, count=fit.count, dbz=att.dbz, zdr=att.zdr, pia=att.pia,
                dphi=att.dphi)


def test_the_two_scenes_differ_everywhere_that_matters():
    a, b = expected("A"), expected("B")
    for key in OUTPUTS:
        assert a[key].shape == b[key].shape and str(a[key].dtype) == OUTPUTS[key]
        assert not np.array_equal(po.bits(a[key]), po.bits(b[key])), key
    assert a["folds"].max() == 1 and b["folds"].max() == 1 and (a["dphi"].max(), b["dphi"].max()) == (120.0, 120.0)
    assert len(set(np.unique(po.half_windows(scene("B")["dbz"], a["kdp"].shape, EDGES, HALF)))) == 3


@pytest.mark.gpu
def test_chain_captured_on_a_replays_on_b_and_on_dirtied_outputs():
    import torch
    import radar_processor_amd as rg
    lib = rg.load_library()
    dev = torch.device("cuda", 0)
    R, G = ps.weather().phidp.shape
    t = {key: torch.empty(value.shape, dtype=getattr(torch, str(value.dtype)), device=dev) for key, value in scene("A").items()}
    out = {key: torch.empty((R, G), dtype=getattr(torch, dtype), device=dev) for key, dtype in OUTPUTS.items()}
    garbage = {key: torch.from_numpy(np.full((R, G), _GARBAGE[dtype], dtype=dtype)).to(dev) for key, dtype in OUTPUTS.items()}
    edges, half = (ctypes.c_double * len(EDGES))(*EDGES), (ctypes.c_int32 * len(HALF))(*HALF)
    P = _native.ptr

    def load(which):
        for key, value in scene(which).items():
            t[key].copy_(torch.from_numpy(np.array(value)))

    def dirty():
        for key, buf in out.items():
            buf.copy_(garbage[key])

    def enqueue(stream):
        return [lib.rg_phidp_unfold_f32(P(t["phidp"]), P(t["mask"]), R, G, WRAP, P(out["unfolded"]), P(out["folds"]), stream),
                lib.rg_phidp_fit_f32(P(out["unfolded"]), R, G, P(t["dbz"]), edges, half, len(HALF), MIN_VALID, 0, SCALE, P(out["kdp"]),
                                     P(out["phi_s"]), P(out["count"]), stream),
                lib.rg_attenuation_phidp_f32(P(out["phi_s"]), P(t["phi0"]), R, G, ALPHA, BETA, MAX_DPHI, P(t["dbz"]), P(t["zdr"]),
                                             P(out["dbz"]), P(out["zdr"]), P(out["pia"]), P(out["dphi"]), stream)]

    def read():
        torch.cuda.synchronize()
        return {key: buf.cpu().numpy() for key, buf in out.items()}

    def check(got, which):
        want = expected(which)
        for key in OUTPUTS:
            np.testing.assert_array_equal(po.bits(got[key]), po.bits(want[key]), err_msg=f"{which}: {key}")

    # eagerly on A and on B: the module is loaded, and these are the results every replay has to equal
    eager = {}
    for which in ("A", "B"):
        load(which)
        dirty()
        assert enqueue(_native.stream_ptr()) == [0, 0, 0], lib.rg_last_error().decode()
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
    assert statuses == [0, 0, 0], lib.rg_last_error().decode()
    for step, which in enumerate(("B", "B", "A", "B")):
        load(which)
        if step != 1:
            dirty()                                                         # step 1: B's own results stand in the outputs
        graph.replay()
        got = read()
        check(got, which)
        for key in got:
            assert got[key].tobytes() == eager[which][key].tobytes(), f"replay {step} on {which}: {key} is not the eager call's"
