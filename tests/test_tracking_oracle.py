"""The tracking scenes and their restatement themselves (tests/tracking_scenes.py, tests/tracking_oracle.py), the host half of
``radar_processor_amd/tracking.py`` against hand-written answers, and the bookkeeping of the ABI -- all on the CPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import motion_oracle as mo
import tracking_oracle as to
import tracking_scenes as ts
import radar_processor_amd as rg
from radar_processor_amd import _native, tracking

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pairs(name):
    s = ts.scene(name)
    return s, to.overlap(s.labels_prev, s.ptr_prev, s.labels_next, s.ptr_next)


# ---- the scenes have the properties they are there for -----------------------------------------------------------------------
def test_one_pair_scenes_hold_every_pixel_in_one_count():
    for name, pixels in (("1x1", 1), ("all_33x65", 33 * 65), ("all_69x199", 69 * 199)):
        s, (a, b, c) = _pairs(name)
        assert s.ptr_prev.tolist() == [0, 1] and s.ptr_next.tolist() == [0, 1]
        assert (a.tolist(), b.tolist(), c.tolist()) == ([0], [0], [pixels])
    assert 65 % 64 and 199 % 64                     # rows end inside a wavefront: the one run goes on across row ends


def test_runs_cross_the_wavefront_seams():
    s, (a, b, c) = _pairs("1x130")
    assert (a.tolist(), b.tolist(), c.tolist()) == ([0, 0], [0, 1], [100, 29])
    nxt = s.labels_next.ravel()
    assert nxt[63] == nxt[64] == 1 and nxt[127] == nxt[128] == 2 and nxt[100] == 0      # a run over index 64, one over 128
    s, (a, b, c) = _pairs("67x1")
    assert s.labels_prev.shape == (1, 67, 1) and c.tolist() == [20, 19, 19, 6] and b.tolist() == [0] * 4
    assert s.labels_prev.ravel()[63] == s.labels_prev.ravel()[64] == 4


def test_checkerboards_are_1024_pairs_of_one_pixel():
    s, (a, b, c) = _pairs("checker_both")
    assert int(s.ptr_prev[-1]) == int(s.ptr_next[-1]) == 1024
    assert a.tolist() == b.tolist() == list(range(1024)) and (c == 1).all()
    s, (a, b, c) = _pairs("checker_vs_all")
    assert int(s.ptr_prev[-1]) == 1024 and int(s.ptr_next[-1]) == 1
    assert a.tolist() == list(range(1024)) and not b.any() and (c == 1).all()


def test_blobs_disjoint_empty_planted_and_stack():
    for t in ts.THRESHOLDS:
        s, (a, b, c) = _pairs(f"blobs_{t}")
        assert len(c) >= 10 and min(int(s.ptr_prev[-1]), int(s.ptr_next[-1])) >= 9
        assert len(set(a.tolist())) < len(a) or len(set(b.tolist())) < len(b)          # some cell has two partners
    s, (a, b, c) = _pairs("disjoint")
    assert len(c) == 0 and int(s.ptr_prev[-1]) > 0 and int(s.ptr_next[-1]) > 0
    s, (a, b, c) = _pairs("empty_next")
    assert len(c) == 0 and int(s.ptr_prev[-1]) > 0 and int(s.ptr_next[-1]) == 0
    s, (a, b, c) = _pairs("planted")
    wild_prev = (s.labels_prev > int(s.ptr_prev[-1])) | (s.labels_prev < 0)
    wild_next = (s.labels_next > int(s.ptr_next[-1])) | (s.labels_next < 0)
    assert wild_prev.sum() >= 100 and wild_next.sum() >= 100
    tame = to.overlap(np.where(wild_prev, 0, s.labels_prev), s.ptr_prev, np.where(wild_next, 0, s.labels_next), s.ptr_next)
    assert all(np.array_equal(x, y) for x, y in zip((a, b, c), tame)) and len(c) > 10
    s, (a, b, c) = _pairs("stack")
    assert s.labels_prev.shape == (2, 69, 199) and s.ptr_next[0] == s.ptr_prev[1] > 0
    assert len(set(np.diff(np.concatenate((s.ptr_prev, s.ptr_next[-1:]))).tolist())) == 3      # three different cell counts
    in_plane = [(s.ptr_prev[p] <= a) & (a < s.ptr_prev[p + 1]) for p in (0, 1)]
    for p in (0, 1):                                # a cell of plane p only meets cells of plane p + 1
        assert in_plane[p].any() and ((b[in_plane[p]] >= s.ptr_next[p]) & (b[in_plane[p]] < s.ptr_next[p + 1])).all()


def test_relabel_and_advect_labels_restatements():
    labels = np.array([[[0, 1, 2], [3, 2, -1]], [[1, 1, 2], [0, 0, 0]]], np.int32)
    ptr = np.array([0, 2, 3], np.int32)
    lut = np.array([10, 20, 30], np.int32)
    assert to.relabel(labels, ptr, lut).tolist() == [[[0, 10, 20], [0, 20, 0]], [[30, 30, 0], [0, 0, 0]]]
    assert to.relabel(labels, ptr, lut[:2]).tolist() == [[[0, 10, 20], [0, 20, 0]], [[0, 0, 0], [0, 0, 0]]]
    assert not to.relabel(labels, ptr, lut[:0]).any()
    plane = np.arange(1, 13, dtype=np.int32).reshape(3, 4)
    field = np.zeros((3, 4, 2), np.float32)
    field[..., 0], field[..., 1] = 1.0, -2.0                                   # echo moves one row up, two columns left
    moved = to.advect_labels(plane, field, mo.Lattice(0.0, 0.0, 1.0, 1.0, 3, 4))
    assert moved.tolist() == [[0, 0, 0, 0], [3, 4, 0, 0], [7, 8, 0, 0]]
    assert to.advect_labels(plane, field, mo.Lattice(0.0, 0.0, 1.0, 1.0, 3, 4), lead=0.0).tobytes() == plane.tobytes()


# ---- match_cells and the identity rules against hand-written answers -------------------------------------------------------
def _overlap(*triples):
    t = np.array(triples, np.int32).reshape(-1, 3)
    return rg.CellOverlap(t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy())


def _both(triples, area_prev, area_next, prev_track, prev_parent, prev_age, next_id, **limits):
    """``(succ, pred, track, parent, age, ended, next_id)`` from the package's host functions, checked against the oracle's
    loops on the way."""
    ov = _overlap(*triples)
    m = rg.match_cells(ov, np.array(area_prev, np.int32), np.array(area_next, np.int32), **limits)
    succ, pred = to.match(ov, area_prev, area_next, limits.get("min_pixels", 1), limits.get("min_fraction", 0.0))
    assert m.succ.dtype == np.int64 and m.pred.dtype == np.int64
    assert m.succ.tolist() == [succ.get(a, -1) for a in range(len(area_prev))]
    assert m.pred.tolist() == [pred.get(b, -1) for b in range(len(area_next))]
    got = tracking.assign_tracks(m, np.array(prev_track, np.int64), np.array(prev_parent, np.int64), np.array(prev_age, np.int64),
                                 next_id)
    want = to.identities(succ, pred, len(area_next), prev_track, prev_parent, prev_age, next_id)
    assert [np.asarray(g).tolist() for g in got[:3]] == [list(w) for w in want[:3]]
    assert got[3].dtype == np.int64 and got[3].shape[1:] == (2,) and got[3].tolist() == [list(e) for e in want[3]]
    assert got[4] == want[4]
    return m.succ.tolist(), m.pred.tolist(), got[0].tolist(), got[1].tolist(), got[2].tolist(), got[3].tolist(), got[4]


def test_continuation_birth_and_death():
    assert _both([(0, 0, 10)], [10], [10], [7], [3], [4], 9) == ([0], [0], [7], [3], [5], [], 9)
    assert _both([(0, 0, 10)], [10], [10, 6], [7], [0], [0], 9) == ([0], [0, -1], [7, 9], [0, 0], [1, 0], [], 10)
    assert _both([(0, 0, 10)], [10, 6], [10], [7, 8], [0, 0], [2, 5], 9) == ([0, -1], [0], [7], [0], [3], [[8, 0]], 9)
    assert _both([], [4, 4], [4], [1, 2], [0, 0], [0, 0], 3) == ([-1, -1], [-1], [3], [0], [0], [[1, 0], [2, 0]], 4)
    assert _both([], [], [], [], [], [], 3) == ([], [], [], [], [], [], 3)


def test_a_split_keeps_the_id_on_the_larger_child():
    # the larger child is row 1: row order does not decide, the count does
    got = _both([(0, 0, 9), (0, 1, 18)], [30], [9, 18], [4], [2], [6], 11)
    assert got == ([1], [0, 0], [11, 4], [4, 2], [0, 7], [], 12)


def test_a_merge_keeps_the_track_of_the_larger_parent():
    got = _both([(0, 0, 7), (1, 0, 20)], [8, 21], [30], [4, 5], [0, 0], [3, 1], 11)
    assert got == ([0, 0], [1], [5], [0], [2], [[4, 5]], 11)


def test_a_count_tie_goes_to_the_smaller_row():
    got = _both([(0, 1, 5), (0, 2, 5), (1, 2, 5), (2, 2, 5)], [9, 9, 9], [9, 9, 9], [1, 2, 3], [0, 0, 0], [0, 0, 0], 4)
    succ, pred = got[:2]
    assert succ == [1, 2, 2] and pred == [-1, 0, 0]
    # row 0 keeps its track in row 1; row 2 of the new frame comes from row 0, whose successor is row 1: a split off track 1
    assert got[2:] == ([4, 1, 5], [0, 0, 1], [0, 1, 0], [[2, 5], [3, 5]], 6)


def test_min_pixels_and_min_fraction_each_flip_one_decision():
    args = ([(0, 0, 3)], [20], [10], [1], [0], [0], 2)
    assert _both(*args, min_pixels=3)[:3] == ([0], [0], [1])
    assert _both(*args, min_pixels=4)[:3] == ([-1], [-1], [2])
    args = ([(0, 0, 5)], [20], [10], [1], [0], [0], 2)                       # the smaller of the two areas is 10
    assert _both(*args, min_fraction=0.5)[:3] == ([0], [0], [1])
    assert _both(*args, min_fraction=0.51)[:3] == ([-1], [-1], [2])
    m = rg.match_cells(_overlap((0, 0, 5), (0, 1, 2)), [20], [10, 10], min_pixels=3)
    assert (m.row_prev.tolist(), m.row_next.tolist(), m.count.tolist()) == ([0], [0], [5])      # the qualifying pairs only


# ---- the four-frame sequence -------------------------------------------------------------------------------------------------
def _motions(frames):
    out = []
    for prev, nxt in zip(frames[:-1], frames[1:]):
        m = mo.block_match(mo.quantize(prev)[None], mo.quantize(nxt)[None], 32, 16, 16)
        out.append((mo.fill_motion(m.motion[0].astype(np.float32), m.score[0].astype(np.float32), 0.5),
                    mo.block_lattice(prev.shape, 32, 16)))
    return out


def test_the_sequence_tells_its_story_and_never_reuses_an_id():
    frames = ts.tracker_frames()
    got = to.track(list(frames), ts.LO, _motions(frames))
    # rows in raster order of each cell's first pixel: A, C, D, F, B | + E | B splits | D merges into C, F has left
    assert [f["track_id"].tolist() for f in got] == [[1, 2, 3, 4, 5], [1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 7, 6], [1, 2, 5, 7, 6]]
    assert [f["parent_track"].tolist() for f in got] == [[0] * 5, [0] * 6, [0, 0, 0, 0, 0, 5, 0], [0, 0, 0, 5, 0]]
    assert [f["age"].tolist() for f in got] == [[0] * 5, [1, 1, 1, 1, 1, 0], [2, 2, 2, 2, 2, 0, 1], [3, 3, 3, 1, 2]]
    assert [f["ended"].tolist() for f in got] == [[], [], [], [[3, 2], [4, 0]]]
    assert got[2]["area"][4] > got[2]["area"][5]                               # the larger child kept track 5
    assert got[2]["area"][1] > got[2]["area"][2]                               # the larger parent's track 2 survives
    assert got[1]["velocity"][0].tolist() == [2.0, -3.0] and np.isnan(got[1]["velocity"][5]).all()
    seen = set()
    for f in got:
        new = f["track_id"][f["age"] == 0].tolist()
        assert not seen & set(new) and (not seen or min(new, default=max(seen) + 1) > max(seen))
        seen |= set(f["track_id"].tolist())


def test_without_advection_a_fast_sequence_loses_its_tracks():
    frames = ts.tracker_frames(ts.FAST_SHIFT)
    moved = to.track(list(frames), ts.LO, _motions(frames))
    still = to.track(list(frames), ts.LO, [None] * 3)
    assert [f["track_id"][0] for f in moved] == [1, 1, 1, 1]                   # blob A, the first cell of every frame
    assert [f["track_id"][0] for f in still] == [1, 6, 10, 14]
    assert max(f["track_id"].max() for f in moved) == 7 and max(f["track_id"].max() for f in still) == 17


# ---- bookkeeping -----------------------------------------------------------------------------------------------------------
FUNCTIONS = ("rg_cell_overlap_workspace_bytes", "rg_cell_overlap_i32", "rg_relabel_cells_i32")
PUBLIC = ("advect_labels_device", "cell_overlap_device", "match_cells", "relabel_cells_device", "CellTracker", "CellOverlap",
          "CellMatch", "TrackFrame")


def test_abi_bookkeeping_and_exports():
    header = open(os.path.join(REPO, "include", "radargrid_hip.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t|const char\*)\s+(rg_\w+)\s*\(", header, flags=re.M))
    assert "#define RG_VERSION 104" in header and _native.ABI_VERSION == 104
    assert "Cell overlap and tracking" in header
    from radar_processor_amd import build
    assert ("rg_tracking.hip", []) in build.SOURCES
    lib = rg.load_library(require_device=False)
    assert lib.rg_version() == 104
    for name in FUNCTIONS:
        restype, argtypes = _native.SIGNATURES[name]
        assert name in declared and getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype
        kind, args = re.search(r"^(int|int64_t) %s\((.*?)\);" % name, header, flags=re.S | re.M).groups()
        assert restype == (ctypes.c_int64 if kind == "int64_t" else ctypes.c_int32)
        want = []
        for a in args.split(","):
            a = " ".join(a.split())
            want.append(ctypes.c_void_p if ("*" in a or a.startswith("rg_stream_t")) else
                        ctypes.c_int64 if a.startswith("int64_t ") else ctypes.c_int32)
        assert want == argtypes, name
    for name in PUBLIC:
        assert name in rg.__all__ and getattr(rg, name) is getattr(tracking, name)


def test_the_first_refusal_of_each_entry_point_needs_no_device():
    lib = rg.load_library(require_device=False)
    assert lib.rg_cell_overlap_workspace_bytes(0) == _native.RG_EINVAL
    assert b"rg_cell_overlap_workspace_bytes: max_pairs" in lib.rg_last_error()
    assert lib.rg_cell_overlap_workspace_bytes(2 ** 30) == _native.RG_EINVAL
    assert lib.rg_cell_overlap_workspace_bytes(1) == 64 * 12 and lib.rg_cell_overlap_workspace_bytes(32) == 64 * 12
    assert lib.rg_cell_overlap_workspace_bytes(33) == 128 * 12 and lib.rg_cell_overlap_workspace_bytes(512) == 1024 * 12
    assert lib.rg_cell_overlap_workspace_bytes(2 ** 30 - 1) == 2 ** 31 * 12
    assert lib.rg_cell_overlap_i32(None, None, None, None, 1, 4, 4, 16, None, None, None, None, 0, None) == _native.RG_EINVAL
    assert b"rg_cell_overlap_i32: null pointer" in lib.rg_last_error()
    assert lib.rg_cell_overlap_i32(None, None, None, None, 0, 4, 4, 16, None, None, None, None, 0, None) == _native.RG_EINVAL
    assert b"rg_cell_overlap_i32: n_planes" in lib.rg_last_error()
    assert lib.rg_cell_overlap_i32(None, None, None, None, 1, 4, 4, 0, None, None, None, None, 0, None) == _native.RG_EINVAL
    assert b"rg_cell_overlap_i32: max_pairs" in lib.rg_last_error()
    assert lib.rg_relabel_cells_i32(None, None, 1, 4, 4, None, 3, None, None) == _native.RG_EINVAL
    assert b"rg_relabel_cells_i32: null pointer" in lib.rg_last_error()
    assert lib.rg_relabel_cells_i32(None, None, 1, 4, -4, None, 3, None, None) == _native.RG_EINVAL
    assert b"rg_relabel_cells_i32: negative size" in lib.rg_last_error()


def test_python_side_validation_comes_before_any_device_use(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched before the arguments were validated")
    for name in ("load_library", "device", "canonical_device", "stream_ptr"):
        monkeypatch.setattr(_native, name, no_device)
    labels = np.zeros((4, 5), np.int32)
    ptr = np.zeros(2, np.int32)
    field = np.zeros((4, 5, 2), np.float32)
    bad_overlap = (dict(labels_prev=labels.astype(np.float32)), dict(labels_next=labels[:3]), dict(labels_next=labels[None]),
                   dict(cell_ptr_prev=np.zeros(3, np.int32)), dict(cell_ptr_next=ptr.astype(np.int64)), dict(max_pairs=0),
                   dict(max_pairs=2 ** 30), dict(max_pairs=2.5), dict(labels_prev=np.zeros((2, 2, 4, 5), np.int32)))
    for kw in bad_overlap:
        args = dict(labels_prev=labels, cell_ptr_prev=ptr, labels_next=labels, cell_ptr_next=ptr, max_pairs=None)
        args.update(kw)
        with pytest.raises(ValueError):
            rg.cell_overlap_device(args["labels_prev"], args["cell_ptr_prev"], args["labels_next"], args["cell_ptr_next"],
                                   max_pairs=args["max_pairs"])
    for call in (lambda: rg.advect_labels_device(labels[None], field), lambda: rg.advect_labels_device(labels.astype(np.int64), field),
                 lambda: rg.advect_labels_device(labels, field[:3]), lambda: rg.advect_labels_device(labels, field, lead=float("nan")),
                 lambda: rg.advect_labels_device(labels, field, substeps=0), lambda: rg.advect_labels_device(labels, field * np.nan),
                 lambda: rg.relabel_cells_device(labels, ptr, np.zeros(3, np.int64)),
                 lambda: rg.relabel_cells_device(labels, np.zeros(3, np.int32), np.zeros(3, np.int32)),
                 lambda: rg.relabel_cells_device(labels.astype(np.uint8), ptr, np.zeros(3, np.int32)),
                 lambda: rg.match_cells(_overlap((0, 0, 1)), [1], [1], min_pixels=0),
                 lambda: rg.match_cells(_overlap((0, 0, 1)), [1], [1], min_fraction=1.5),
                 lambda: rg.match_cells(_overlap((0, 3, 1)), [1], [1]),
                 lambda: rg.CellTracker(float("nan")), lambda: rg.CellTracker(35.0, connectivity=6),
                 lambda: rg.CellTracker(35.0, min_size=0), lambda: rg.CellTracker(35.0, min_pixels=0),
                 lambda: rg.CellTracker(35.0, min_fraction=-0.1), lambda: rg.CellTracker(35.0, motion="fast"),
                 lambda: rg.CellTracker(35.0, blocks=8), lambda: rg.CellTracker(35.0, block=7),
                 lambda: rg.CellTracker(35.0, motion=None, block=8),
                 lambda: rg.CellTracker(35.0).update(np.zeros((4, 5), np.float64)),
                 lambda: rg.CellTracker(35.0).update(np.zeros((1, 4, 5), np.float32))):
        with pytest.raises(ValueError):
            call()
    frame = rg.TrackFrame(None, None, None, None, np.array([2 ** 31], np.int64), np.zeros(1, np.int64), np.zeros(1, np.int64),
                          np.zeros((1, 2)), np.zeros((0, 2), np.int64))
    with pytest.raises(OverflowError):
        frame.track_plane_device()
