"""Host-only halves of the stream contract (include/radargrid_hip.h: "no global mutable state: entry points are thread-safe per
stream"): the table of tests/test_gpu_graph_replay.py names every entry point that takes a stream, and ``rg_last_error`` is
each thread's own.  No device is touched: the refusals used here return before any HIP call, as
tests/test_rowwise_entry_refusals.py relies on."""
import ctypes
import threading

import radar_processor_amd as rg
from radar_processor_amd import _native

import test_gpu_graph_replay as replay

P = 1 << 12                                  # an aligned address that is never dereferenced


def stream_taking():
    """Every bound function whose last argument is the stream: in the header that is exactly the functions with an
    ``rg_stream_t``, and ``_native.SIGNATURES`` mirrors the header one to one."""
    return {name for name, (_, argtypes) in _native.SIGNATURES.items() if argtypes and argtypes[-1] is ctypes.c_void_p}


def test_every_entry_point_that_takes_a_stream_is_chained_or_excluded_with_a_reason():
    chained = [name for names in replay.CHAINED.values() for name in names]
    assert len(chained) == len(set(chained)) and not set(chained) & set(replay.EXCLUDED)
    assert all(isinstance(reason, str) and len(reason) > 20 for reason in replay.EXCLUDED.values())
    listed = set(chained) | set(replay.EXCLUDED)
    assert listed == stream_taking(), (sorted(stream_taking() - listed), sorted(listed - stream_taking()))
    assert set(replay.CHAINED) == set(replay.BUILDERS) and len(stream_taking()) >= 60
    assert not any(name.endswith("_bytes") for name in listed)


def test_rg_last_error_is_each_threads_own():
    """Two threads take turns through a barrier, each refusing another entry point for another reason; each always reads its
    own message back, and a third thread that never had an error reads the empty string."""
    lib = rg.load_library(require_device=False)
    rounds = 50
    barrier = threading.Barrier(2)
    seen = {"overlap": [], "relabel": [], "quiet": None}

    def overlap():
        for k in range(rounds):
            barrier.wait(timeout=30)
            status = lib.rg_cell_overlap_i32(P, P, P, P, 0, 4, 5, 8, P, P, P, P, 768, None)          # n_planes = 0
            barrier.wait(timeout=30)                                                                  # the other thread has failed too
            seen["overlap"].append((status, lib.rg_last_error()))

    def relabel():
        for k in range(rounds):
            barrier.wait(timeout=30)
            status = lib.rg_relabel_cells_i32(P, P, 2, 4, 5, P, -1 - k, P + (1 << 20), None)         # n_cells negative, another each round
            barrier.wait(timeout=30)
            seen["relabel"].append((status, lib.rg_last_error()))

    def quiet():
        seen["quiet"] = lib.rg_last_error()

    threads = [threading.Thread(target=f) for f in (overlap, relabel)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=120)
    assert not any(th.is_alive() for th in threads)
    third = threading.Thread(target=quiet)
    third.start()
    third.join(timeout=30)
    assert len(seen["overlap"]) == len(seen["relabel"]) == rounds
    for status, message in seen["overlap"]:
        assert status == _native.RG_EINVAL and message == b"rg_cell_overlap_i32: n_planes must be at least 1, got 0", message
    for k, (status, message) in enumerate(seen["relabel"]):
        assert status == _native.RG_EINVAL and message == b"rg_relabel_cells_i32: negative n_cells %d" % (-1 - k), message
    assert seen["quiet"] == b""
