"""Cell overlap, relabelling, label advection and the tracker on the GPU (csrc/rg_tracking.hip, radar_processor_amd/tracking.py)
against the NumPy restatement of tests/tracking_oracle.py, through the public functions and through the raw C ABI.

Every output is an integer (the velocities are quotients of integers formed the same way on both sides), so every comparison
is exact.  Scenes: tests/tracking_scenes.py, nothing above 69 x 199."""
import functools

import numpy as np
import pytest

import motion_oracle as mo
import tracking_oracle as to
import tracking_scenes as ts

pytestmark = pytest.mark.gpu
CANARY = 64


@pytest.fixture(scope="module")
def env():
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native
    lib = rg.load_library()
    return dict(torch=torch, rg=rg, native=_native, lib=lib, dev=torch.device("cuda", 0))


@functools.lru_cache(maxsize=None)
def reference(name):
    s = ts.scene(name)
    out = to.overlap(s.labels_prev, s.ptr_prev, s.labels_next, s.ptr_next)
    for a in out:
        a.setflags(write=False)
    return out


def _dev(env, a):
    return env["torch"].from_numpy(np.array(a)).to(env["dev"])


def _lut(n):
    return (np.arange(n, dtype=np.int64) * 2654435761 % 1000003 - 500000).astype(np.int32)      # any integers, negative too


# ---- overlap through the public call -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ts.NAMES)
def test_overlap_equals_the_oracle_and_repeats(env, name):
    rg, s = env["rg"], ts.scene(name)
    args = [_dev(env, a) for a in s[1:]]
    got = rg.cell_overlap_device(*args)
    want = reference(name)
    print(f"{name}: {len(want[2])} pairs, largest {int(want[2].max(initial=0))} pixels")
    for g, w, what in zip(got, want, ("row_prev", "row_next", "count")):
        g = g.cpu().numpy()
        assert g.dtype == np.int32 and g.shape == w.shape, what
        np.testing.assert_array_equal(g, w, err_msg=f"{name}: {what}")
    again = rg.cell_overlap_device(*args)
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(got, again))
    if s.labels_prev.shape[0] == 1:                                            # 2-D planes and ndarrays go the same way
        flat = rg.cell_overlap_device(s.labels_prev[0], s.ptr_prev, s.labels_next[0], s.ptr_next)
        assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(got, flat))


def test_an_explicit_max_pairs_that_is_too_small_raises(env):
    rg, s = env["rg"], ts.scene("checker_both")
    args = [_dev(env, a) for a in s[1:]]
    assert len(rg.cell_overlap_device(*args, max_pairs=1024).count) == 1024
    with pytest.raises(RuntimeError, match=r"max_pairs = 512 .* holds 1024 distinct pairs and 0 insertion"):
        rg.cell_overlap_device(*args, max_pairs=512)
    with pytest.raises(RuntimeError, match=r"max_pairs = 256 .* holds 512 distinct pairs and [1-9]\d* insertion"):
        rg.cell_overlap_device(*args, max_pairs=256)


# ---- overlap through the raw ABI ---------------------------------------------------------------------------------------------
def _guarded(env, n, dtype, pattern):
    """A buffer of n elements between two canaries of CANARY elements, filled with ``pattern``; returns (buffer, view)."""
    buf = env["torch"].full((2 * CANARY + n,), pattern, dtype=dtype, device=env["dev"])
    return buf, buf[CANARY:CANARY + n]


def _intact(buf, n, pattern):
    host = buf.cpu().numpy()
    return bool((host[:CANARY] == pattern).all() and (host[CANARY + n:] == pattern).all())


def _raw_overlap(env, name, max_pairs, short=0):
    """One rg_cell_overlap_i32 call into guarded buffers: (status, totals, written triples as a set, canaries intact)."""
    torch, nat, lib = env["torch"], env["native"], env["lib"]
    s = ts.scene(name)
    n, h, w = s.labels_prev.shape
    lp, pp, ln, pn = (_dev(env, a) for a in s[1:])
    need = int(lib.rg_cell_overlap_workspace_bytes(max_pairs))
    cap = 64
    while cap < 2 * max_pairs:
        cap *= 2
    assert need == 12 * cap
    rows_buf, rows = _guarded(env, 2 * max_pairs, torch.int32, -77)
    count_buf, count = _guarded(env, max_pairs, torch.int32, -77)
    totals_buf, totals = _guarded(env, 2, torch.int32, -77)
    ws_buf, ws = _guarded(env, need // 8, torch.int64, -77)               # 64 int64 canaries: 8-byte aligned behind them
    with torch.cuda.device(env["dev"]):
        status = lib.rg_cell_overlap_i32(nat.ptr(lp), nat.ptr(pp), nat.ptr(ln), nat.ptr(pn), n, h, w, max_pairs, nat.ptr(rows),
                                         nat.ptr(count), nat.ptr(totals), nat.ptr(ws), need - short, nat.stream_ptr())
    torch.cuda.synchronize()
    intact = (_intact(rows_buf, 2 * max_pairs, -77) and _intact(count_buf, max_pairs, -77) and _intact(totals_buf, 2, -77)
              and _intact(ws_buf, need // 8, -77))
    t = totals.cpu().numpy().tolist()
    if status != 0:
        return status, t, set(), intact, rows.cpu().numpy(), count.cpu().numpy()
    k = min(t[0], max_pairs)
    r, c = rows.cpu().numpy().reshape(-1, 2), count.cpu().numpy()
    assert (r[k:] == -77).all() and (c[k:] == -77).all()                       # only min(totals[0], max_pairs) entries are written
    return status, t, {(int(a), int(b), int(v)) for (a, b), v in zip(r[:k], c[:k])}, intact, r, c


def test_raw_abi_full_tables_canaries_and_a_short_workspace(env):
    nat = env["native"]
    want = {(int(a), int(b), int(c)) for a, b, c in zip(*reference("checker_both"))}
    assert len(want) == 1024
    status, totals, got, intact, _, _ = _raw_overlap(env, "checker_both", 1024)
    assert status == 0 and totals == [1024, 0] and got == want and intact
    # C = 1024 slots for 1024 pairs: the table is 100 % full, nothing is dropped, 512 entries come out
    status, totals, got, intact, _, _ = _raw_overlap(env, "checker_both", 512)
    assert status == 0 and totals == [1024, 0] and len(got) == 512 and got <= want and intact
    # C = 512: half the pairs find the table full
    status, totals, got, intact, _, _ = _raw_overlap(env, "checker_both", 256)
    print(f"max_pairs 256: totals {totals}")
    assert status == 0 and totals[0] == 512 and totals[1] > 0 and len(got) == 256 and got <= want and intact
    assert totals[1] == 1024 - 512                                            # every pair is one pixel: one insertion each
    # one slot takes every insertion; a table far larger than the pairs
    for name, max_pairs in (("all_69x199", 1), ("blobs_0.55", 5000), ("stack", 85), ("planted", 64)):
        want_n = {(int(a), int(b), int(c)) for a, b, c in zip(*reference(name))}
        status, totals, got, intact, _, _ = _raw_overlap(env, name, max_pairs)
        assert status == 0 and totals == [len(want_n), 0] and got == want_n and intact, name
    status, totals, got, intact, r, c = _raw_overlap(env, "checker_both", 1024, short=1)
    assert status == nat.RG_EWORKSPACE and intact and totals == [-77, -77] and (r == -77).all() and (c == -77).all()
    assert b"rg_cell_overlap_i32: workspace of 24575 bytes, 24576 needed" in env["lib"].rg_last_error()


def test_raw_abi_refusals_and_empty_planes(env):
    torch, nat, lib = env["torch"], env["native"], env["lib"]
    dev = env["dev"]
    lab = torch.ones((2, 4, 5), dtype=torch.int32, device=dev)
    lab2 = torch.ones((2, 4, 5), dtype=torch.int32, device=dev)
    ptr = torch.tensor([0, 1, 2], dtype=torch.int32, device=dev)
    ptr2 = ptr.clone()
    rows = torch.full((16, 2), -77, dtype=torch.int32, device=dev)
    count = torch.full((16,), -77, dtype=torch.int32, device=dev)
    totals = torch.full((2,), -77, dtype=torch.int32, device=dev)
    ws = torch.zeros(96, dtype=torch.int64, device=dev)

    def call(**kw):
        d = dict(lp=nat.ptr(lab), pp=nat.ptr(ptr), ln=nat.ptr(lab2), pn=nat.ptr(ptr2), n=2, h=4, w=5, max_pairs=8,
                 rows=nat.ptr(rows), count=nat.ptr(count), totals=nat.ptr(totals), ws=nat.ptr(ws), ws_bytes=768)
        d.update(kw)
        with torch.cuda.device(dev):
            return lib.rg_cell_overlap_i32(*d.values(), nat.stream_ptr())

    assert call() == 0
    assert totals.cpu().tolist() == [2, 0]
    assert sorted(zip(rows[:2].cpu().tolist(), count[:2].cpu().tolist())) == [([0, 0], 20), ([1, 1], 20)]
    for kw, message in ((dict(lp=0), "null pointer"), (dict(pp=0), "null pointer"), (dict(ln=0), "null pointer"),
                        (dict(pn=0), "null pointer"), (dict(rows=0), "null pointer"), (dict(count=0), "null pointer"),
                        (dict(totals=0), "null pointer"), (dict(ws=0), "null pointer"), (dict(n=0), "n_planes must be at least 1"),
                        (dict(h=-1), "negative size"), (dict(w=-1), "negative size"),
                        (dict(n=2, h=32768, w=32768), "2^31 pixels or more"), (dict(max_pairs=0), "max_pairs must lie in"),
                        (dict(max_pairs=2 ** 30), "max_pairs must lie in"), (dict(rows=nat.ptr(lab) + 8), "overlaps an input"),
                        (dict(count=nat.ptr(lab2)), "overlaps an input"), (dict(totals=nat.ptr(ptr) + 4), "overlaps an input"),
                        (dict(ws=nat.ptr(lab2) + 16), "overlaps an input")):
        assert call(**kw) == nat.RG_EINVAL, kw
        assert lib.rg_last_error().decode().startswith("rg_cell_overlap_i32: ") and message in lib.rg_last_error().decode(), kw
    assert call(ws_bytes=767) == nat.RG_EWORKSPACE and call(ws=nat.ptr(ws) + 4) == nat.RG_EALIGN
    assert call(max_pairs=33) == nat.RG_EWORKSPACE                              # 128 slots need 1536 bytes
    totals.fill_(-77)
    rows.fill_(-77)
    assert call(h=0) == 0 and totals.cpu().tolist() == [0, 0] and (rows == -77).all()
    totals.fill_(-77)
    assert call(w=0) == 0 and totals.cpu().tolist() == [0, 0]
    assert call(lp=nat.ptr(lab), ln=nat.ptr(lab), pp=nat.ptr(ptr), pn=nat.ptr(ptr)) == 0       # the inputs may be one array
    assert totals.cpu().tolist() == [2, 0]
    out = torch.zeros((2, 4, 5), dtype=torch.int32, device=dev)
    lut = torch.tensor([5, 6], dtype=torch.int32, device=dev)

    def relabel(**kw):
        d = dict(lab=nat.ptr(lab), ptr=nat.ptr(ptr), n=2, h=4, w=5, lut=nat.ptr(lut), cells=2, out=nat.ptr(out))
        d.update(kw)
        with torch.cuda.device(dev):
            return lib.rg_relabel_cells_i32(*d.values(), nat.stream_ptr())

    assert relabel() == 0 and out[0].eq(5).all() and out[1].eq(6).all()
    for kw, message in ((dict(lab=0), "null pointer"), (dict(ptr=0), "null pointer"), (dict(out=0), "null pointer"),
                        (dict(lut=0), "null pointer"), (dict(n=0), "n_planes must be at least 1"), (dict(h=-1), "negative size"),
                        (dict(n=2, h=32768, w=32768), "2^31 pixels or more"), (dict(cells=-1), "negative n_cells"),
                        (dict(out=nat.ptr(lab) + 4), "out overlaps labels"), (dict(out=nat.ptr(out), lut=nat.ptr(out) + 8), "cell_ptr or lut")):
        assert relabel(**kw) == nat.RG_EINVAL, kw
        assert lib.rg_last_error().decode().startswith("rg_relabel_cells_i32: ") and message in lib.rg_last_error().decode(), kw
    assert relabel(lut=0, cells=0) == 0 and not out.any()                       # no cells: zeros, the table may be NULL
    assert relabel(h=0) == 0
    torch.cuda.synchronize()


# ---- relabel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ts.NAMES)
def test_relabel_equals_the_oracle_in_place_too(env, name):
    torch, nat, lib, rg = env["torch"], env["native"], env["lib"], env["rg"]
    s = ts.scene(name)
    for labels, ptr in ((s.labels_prev, s.ptr_prev), (s.labels_next, s.ptr_next)):
        cells = int(ptr[-1])                                                   # rows of the stack's table, not only this view's
        for lut in (_lut(cells), _lut(cells)[:cells // 2], _lut(0)):           # a table that is too short; no cells at all
            want = to.relabel(labels, ptr, lut)
            got = rg.relabel_cells_device(_dev(env, labels), _dev(env, ptr), _dev(env, lut))
            assert got.dtype == torch.int32 and got.cpu().numpy().tobytes() == want.tobytes(), (name, len(lut))
        lut = _lut(cells)
        n, h, w = labels.shape
        buf, view = _guarded(env, labels.size, torch.int32, -77)
        view.copy_(torch.from_numpy(labels.ravel().copy()))
        with torch.cuda.device(env["dev"]):
            assert lib.rg_relabel_cells_i32(nat.ptr(view), nat.ptr(_dev(env, ptr)), n, h, w, nat.ptr(_dev(env, lut)), cells,
                                            nat.ptr(view), nat.stream_ptr()) == 0
        assert view.cpu().numpy().tobytes() == to.relabel(labels, ptr, lut).tobytes() and _intact(buf, labels.size, -77)


# ---- advect_labels ---------------------------------------------------------------------------------------------------------
def test_advect_labels_equals_the_oracle(env):
    rg = env["rg"]
    labels = ts.scene("blobs_0.55").labels_prev[0]
    h, w = labels.shape
    dense = np.empty((h, w, 2), np.float32)
    dense[..., 0], dense[..., 1] = 2.25, -3.5                                  # constant, one vector per pixel
    yy, xx = np.mgrid[0:5, 0:7]
    shear = np.stack([0.75 * xx - 1.5, 4.0 - 1.25 * yy], axis=-1).astype(np.float32)            # sheared, on a coarse lattice
    lattice = mo.Lattice(-3.0, 2.5, 17.0, 31.5, 5, 7)
    for field, lat, kw in ((dense, None, {}), (shear, lattice, {}), (shear, lattice, dict(lead=2.5, substeps=3))):
        got = rg.advect_labels_device(_dev(env, labels), _dev(env, field), lattice=lat, **kw)
        want = to.advect_labels(labels, field, lat or mo.Lattice(0.0, 0.0, 1.0, 1.0, h, w), kw.get("lead", 1.0), kw.get("substeps", 1))
        assert got.dtype == env["torch"].int32 and tuple(got.shape) == (h, w)
        assert got.cpu().numpy().tobytes() == want.tobytes()
        assert (want != labels).any() and want.any()
    assert rg.advect_labels_device(labels, shear, lattice=lattice, lead=0.0).cpu().numpy().tobytes() == labels.tobytes()


# ---- the tracker -----------------------------------------------------------------------------------------------------------
def _run(env, frames, **kw):
    tracker = env["rg"].CellTracker(ts.LO, **kw)
    return tracker, [tracker.update(_dev(env, f)) for f in frames]


def _check_frames(env, got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g.labels.cpu().numpy(), w["labels"][0], err_msg=f"frame {k}: labels")
        np.testing.assert_array_equal(g.cell_ptr.cpu().numpy(), w["cell_ptr"])
        for name in ("track_id", "parent_track", "age", "ended"):
            assert getattr(g, name).dtype == np.int64
            np.testing.assert_array_equal(getattr(g, name), w[name], err_msg=f"frame {k}: {name}")
        assert g.velocity.dtype == np.float64 and g.velocity.shape == (len(w["track_id"]), 2)
        assert g.velocity.tobytes() == w["velocity"].tobytes(), f"frame {k}: velocity"
        np.testing.assert_array_equal(g.table.area.cpu().numpy(), w["area"])
        plane = g.track_plane_device()
        assert plane.dtype == env["torch"].int32
        np.testing.assert_array_equal(plane.cpu().numpy(), to.relabel(w["labels"], w["cell_ptr"], w["track_id"].astype(np.int32))[0])


def _motions(got, shape):
    """The filled motion each frame was matched along, as the oracle takes it."""
    lat = mo.block_lattice(shape, 32, 16)
    assert got[0].motion is None
    for g in got[1:]:
        assert tuple(g.motion.lattice) == tuple(lat)
    return [(g.motion.motion.cpu().numpy(), lat) for g in got[1:]]


def test_tracker_follows_the_sequence(env):
    frames = ts.tracker_frames()
    tracker, got = _run(env, frames)
    want = to.track(list(frames), ts.LO, _motions(got, frames[0].shape))
    _check_frames(env, got, want)
    # the story of tests/tracking_scenes.py: A, C, D, F, B; E is born; B splits; D merges into C and F has left
    assert [g.track_id.tolist() for g in got] == [[1, 2, 3, 4, 5], [1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 7, 6], [1, 2, 5, 7, 6]]
    assert got[2].parent_track.tolist() == [0, 0, 0, 0, 0, 5, 0] and got[3].ended.tolist() == [[3, 2], [4, 0]]
    assert got[3].age.tolist() == [3, 3, 3, 1, 2] and tracker.next_id == 8
    assert got[1].velocity[0].tolist() == [2.0, -3.0] and np.isnan(got[1].velocity[5]).all()


def test_tracker_needs_advection_for_a_fast_sequence(env):
    frames = ts.tracker_frames(ts.FAST_SHIFT)
    moving, got = _run(env, frames)
    _check_frames(env, got, to.track(list(frames), ts.LO, _motions(got, frames[0].shape)))
    for g in got[1:]:                                                         # the estimate is the shift the frames were built with
        mean = g.motion.motion.cpu().numpy().reshape(-1, 2).mean(axis=0)
        assert abs(mean[0] - ts.FAST_SHIFT[0]) <= 1.0 and abs(mean[1] - ts.FAST_SHIFT[1]) <= 1.0
    assert [int(g.track_id[0]) for g in got] == [1, 1, 1, 1] and moving.next_id == 8
    # the same frames compared where they are: every blob is further away than it is wide, and blob A starts over every frame
    standing, lost = _run(env, frames, motion=None)
    _check_frames(env, lost, to.track(list(frames), ts.LO, [None] * 3))
    assert all(g.motion is None for g in lost)
    assert [int(g.track_id[0]) for g in lost] == [1, 6, 10, 14] and standing.next_id == 18
    assert all((g.age[0] == 0) and np.isnan(g.velocity[0]).all() for g in lost)


def test_tracker_takes_a_given_field_and_despeckles(env):
    frames = ts.tracker_frames()
    h, w = frames[0].shape
    field = np.empty((h, w, 2), np.float32)
    field[..., 0], field[..., 1] = ts.SHIFT
    _, got = _run(env, frames[:3], motion=_dev(env, field))
    want = to.track(list(frames[:3]), ts.LO, [(field, mo.Lattice(0.0, 0.0, 1.0, 1.0, h, w))] * 2)
    _check_frames(env, got, want)
    # min_size 30 removes D (29 pixels) and F before they become cells
    _, got = _run(env, frames[:2], min_size=30, motion=None)
    assert [g.table.area.cpu().tolist() for g in got] == [[113, 81, 116], [113, 81, 116, 81]]
    assert [g.track_id.tolist() for g in got] == [[1, 2, 3], [1, 2, 3, 4]]
