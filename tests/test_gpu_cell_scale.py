"""The cell kernels (csrc/rg_components.hip, csrc/rg_tracking.hip) at the sizes where a trip count or a magnitude depends on
size, against tests/components_oracle.py and tests/tracking_oracle.py as they stand and, for the 100 000-pixel lines, against
closed forms.  Scenes: tests/cell_scale_scenes.py; tests/test_cell_scale_scenes.py proves on the CPU that each one reaches
the path named here.

``many_planes``   600 chunks: three trips of ``cc_scan_kernel``, ``cell_ptr`` written in every trip, ten plane boundaries per
                  wavefront in ``cell_of`` / ``row_of`` / ``run_of`` / ``run_of_pair`` with equal labels on both sides;
``straddle``      the second scan trip starts in the middle of plane 85: ``offsets[chunk] - offsets[p * chunks]`` of
                  ``cc_rank_kernel`` across the carry;
``one_big``       263 chunks and 153 tiles in one plane: cells that percolate through most tiles, one cell of 134 000 pixels,
                  134 000 cells of one pixel (``cc_stats_init_kernel`` / ``cc_stats_finish_kernel`` over 526 workgroups; the
                  overlap table with 134 000 keys);
``long_*``        index sums of 4 999 950 000: the carry of the 64-bit atomic add into the high word of ``sum_yx``; 1563 tiles
                  side by side and 3125 on top of each other.

Every comparison is exact (``vmax`` bitwise) except ``vsum``: ``|vsum - fsum| <= area * 2^-53 * sum|v|``, the bound of
tests/test_gpu_components.py, whose ``_check_table`` is imported.  The many-planes scenes run first, then ``straddle``, then
the rest: if a later scan trip is wrong, the smallest input shows it.

What no scene of a few megabytes can reach: the index sums INSIDE a wavefront.  A wavefront's final sum is 64 coordinates, the
widest partial sum that goes through ``shfl_up_i64`` is 32 coordinates (the last step of the scan), so the high half of that
shuffle is zero in every scene above, and only the atomic accumulation crosses 2^32.  The last test of the file therefore builds
one line of 2^27 + 2^21 pixels ON THE DEVICE (1.02 GiB there, nothing on the host, nothing to label) and asks for ``area`` and
``sum_yx`` alone, whose answers are closed forms.

Out of scope: the host loops that split a call into several launches (``kPerLaunch``, ``kTilesPerLaunch`` in rg_warp.hip and
rg_georef.hip) -- a second launch needs 2^31 elements; and the block-match kernel, whose size-dependent paths (more than 256
candidates per block, all four byte shifts, odd R, B = 64 with R = 32) tests/test_gpu_motion.py drives with ``extremes_64_32``
and ``rim``."""
import functools

import numpy as np
import pytest

import cell_scale_scenes as css
import components_oracle as co
import tracking_oracle as to
from test_gpu_components import _check_table

pytestmark = pytest.mark.gpu
EXACT = ("plane", "id", "area", "bbox", "sum_yx", "argmax")


@pytest.fixture(scope="module")
def env():
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native
    lib = rg.load_library()
    return dict(torch=torch, rg=rg, native=_native, lib=lib, dev=torch.device("cuda", 0))


@functools.lru_cache(maxsize=None)
def reference_table(name, connectivity):
    """The cell table of one case, computed once: ``co.stats`` where it is affordable, the closed form for the lines, the
    vectorised restatement (no ``vsum``) for the rest.  Read-only."""
    s = css.scene(name)
    labels, cell_ptr = css.labelled(name, connectivity)
    if name.startswith("long_"):
        table = css.line_expected(name)[2]
    elif (name, connectivity) in css.FULL_TABLE_CASES:
        table = co.stats(s.planes, labels, cell_ptr)
    else:
        table = css.vector_table(s.planes, labels, cell_ptr)
    for a in table.values():
        a.setflags(write=False)
    return table


@functools.lru_cache(maxsize=None)
def reference_overlap(name):
    out = to.overlap(*css.overlap_scene(name)[1:])
    for a in out:
        a.setflags(write=False)
    return out


def _dev(env, a):
    return env["torch"].from_numpy(np.array(a)).to(env["dev"])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _lut(n):
    return (np.arange(n, dtype=np.int64) * 2654435761 % 1000003 - 500000).astype(np.int32)      # any integers, negative too


# ---- labelling ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", css.CASES, ids=css.case_id)
def test_labels_and_cell_ptr_equal_the_oracle_and_repeat(env, case):
    rg = env["rg"]
    name, connectivity = case
    s = css.scene(name)
    want_labels, want_ptr = css.labelled(name, connectivity)
    planes = _dev(env, s.planes)
    runs = []
    for _ in range(2):
        labels, cell_ptr = rg.label_components_device(planes, s.lo, upper=s.hi, connectivity=connectivity, wrap_rows=s.wrap)
        runs.append((labels.cpu().numpy(), cell_ptr.cpu().numpy()))
    labels, cell_ptr = runs[0]
    print(f"{css.case_id(case)}: planes {tuple(s.planes.shape)}, {css.chunks_of(s.planes.shape)} chunks, "
          f"{css.scan_trips(s.planes.shape)} scan trips, {int(want_ptr[-1])} cells")
    assert labels.dtype == np.int32 and cell_ptr.dtype == np.int32 and labels.shape == s.planes.shape
    np.testing.assert_array_equal(cell_ptr, want_ptr, err_msg=f"{case}: cell_ptr")
    np.testing.assert_array_equal(labels, want_labels, err_msg=f"{case}: labels")
    assert runs[1][0].tobytes() == labels.tobytes() and runs[1][1].tobytes() == cell_ptr.tobytes(), f"{case}: second run"
    assert planes.cpu().numpy().tobytes() == s.planes.tobytes()                                   # the input is untouched


# ---- the cell table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", css.CASES, ids=css.case_id)
def test_cell_table_equals_the_reference(env, case):
    """From the reference labelling, so that a wrong table is the table kernels' doing.  The full comparison of
    ``_check_table`` where the oracle can afford it and on the lines; everything but ``vsum`` on the others."""
    rg = env["rg"]
    name, connectivity = case
    s = css.scene(name)
    labels, cell_ptr = css.labelled(name, connectivity)
    want = reference_table(name, connectivity)
    table = rg.cell_table_device(_dev(env, s.planes), _dev(env, labels), _dev(env, cell_ptr))
    got = {k: v.cpu().numpy() for k, v in table._asdict().items() if v is not None}
    print(f"{css.case_id(case)}: {css.chunks_of(s.planes.shape)} chunks, {css.scan_trips(s.planes.shape)} scan trips, "
          f"{int(cell_ptr[-1])} cells, largest cell {int(want['area'].max())} pixels, largest sum_yx entry "
          f"{int(want['sum_yx'].max())}, largest on the device {int(got['sum_yx'].max())}")
    assert len(got["area"]) == int(cell_ptr[-1])
    for column in EXACT:
        assert got[column].dtype == want[column].dtype, column
        np.testing.assert_array_equal(got[column], want[column], err_msg=f"{case}: {column}")
    np.testing.assert_array_equal(_bits(got["vmax"]), _bits(want["vmax"]), err_msg=f"{case}: vmax bits")
    if "vsum" in want:
        _check_table(got, want, css.case_id(case))
    else:
        assert labels.shape[0] == 1 and (name, connectivity) not in css.FULL_TABLE_CASES
        cells = int(cell_ptr[-1])
        np.testing.assert_array_equal(got["area"], np.bincount(labels.ravel(), minlength=cells + 1)[1:], err_msg=f"{case}: area")
        assert not got["plane"].any() and got["id"].tolist() == list(range(1, cells + 1))         # what cell_ptr = [0, cells] says


# ---- despeckle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", css.DESPECKLE_CASES, ids=css.case_id)
def test_despeckle_equals_the_oracle_bytewise(env, case):
    """``area[cell_ptr[i / hw] + l - 1]`` over many planes, and over one plane of many chunks."""
    rg, torch = env["rg"], env["torch"]
    name, connectivity = case
    s = css.scene(name)
    labels, cell_ptr = css.labelled(name, connectivity)
    largest = int(reference_table(name, connectivity)["area"].max())
    planes = _dev(env, s.planes)
    for min_size, fill in ((2, -9.25), (largest, np.nan)):
        want, want_removed = co.despeckle_labelled(s.planes, labels, cell_ptr, min_size, fill)
        out, removed = rg.despeckle_device(planes, s.lo, min_size, upper=s.hi, connectivity=connectivity, wrap_rows=s.wrap,
                                           fill_value=fill, return_mask=True)
        print(f"{css.case_id(case)} min_size {min_size}: {int(want_removed.sum())} pixels removed")
        assert out.shape == planes.shape and out.dtype == torch.float32 and removed.dtype == torch.uint8
        assert out.cpu().numpy().tobytes() == want.tobytes(), (case, min_size)
        assert removed.cpu().numpy().tobytes() == want_removed.tobytes(), (case, min_size)
        assert 0 < int(want_removed.sum()) < int((labels > 0).sum())                               # some cells go, some stay
    assert planes.cpu().numpy().tobytes() == s.planes.tobytes()


# ---- overlap and relabel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", css.OVERLAP_NAMES)
def test_overlap_equals_the_oracle_and_repeats(env, name):
    rg, s = env["rg"], css.overlap_scene(name)
    args = [_dev(env, a) for a in s[1:]]
    got = rg.cell_overlap_device(*args)                                       # the default max_pairs: at most half full
    want = reference_overlap(name)
    print(f"{name}: planes {tuple(s.labels_prev.shape)}, {len(want[2])} pairs, largest {int(want[2].max())} pixels")
    for g, w, what in zip(got, want, ("row_prev", "row_next", "count")):
        g = g.cpu().numpy()
        assert g.dtype == np.int32 and g.shape == w.shape, what
        np.testing.assert_array_equal(g, w, err_msg=f"{name}: {what}")
    again = rg.cell_overlap_device(*args)
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(got, again))


@pytest.mark.parametrize("name", css.OVERLAP_NAMES)
def test_relabel_equals_the_oracle(env, name):
    rg, torch, s = env["rg"], env["torch"], css.overlap_scene(name)
    for labels, ptr in ((s.labels_prev, s.ptr_prev), (s.labels_next, s.ptr_next)):
        cells = int(ptr[-1])
        labels_t, ptr_t = _dev(env, labels), _dev(env, ptr)
        for lut in (_lut(cells), _lut(cells)[:cells // 2]):                    # the whole table; one that is too short
            want = to.relabel(labels, ptr, lut)
            got = rg.relabel_cells_device(labels_t, ptr_t, _dev(env, lut))
            assert got.dtype == torch.int32 and got.cpu().numpy().tobytes() == want.tobytes(), (name, len(lut))


def test_raw_overlap_with_exactly_as_many_pairs_as_max_pairs(env):
    """134 420 one-pixel cells against one cell through ``rg_cell_overlap_i32`` with ``max_pairs`` equal to the pair count:
    every pair comes out, nothing is dropped, nothing is written beyond them."""
    torch, nat, lib = env["torch"], env["native"], env["lib"]
    s = css.overlap_scene("checker_vs_all")
    want = reference_overlap("checker_vs_all")
    pairs = len(want[2])
    n, h, w = s.labels_prev.shape
    lp, pp, ln, pn = (_dev(env, a) for a in s[1:])
    need = int(lib.rg_cell_overlap_workspace_bytes(pairs))
    assert need % 12 == 0 and need // 12 >= 2 * pairs                          # 2^19 slots: the table is at most half full
    rows = torch.full((pairs + 64, 2), -77, dtype=torch.int32, device=env["dev"])
    count = torch.full((pairs + 64,), -77, dtype=torch.int32, device=env["dev"])
    totals = torch.full((2,), -77, dtype=torch.int32, device=env["dev"])
    workspace = torch.empty(need // 8, dtype=torch.int64, device=env["dev"])
    with torch.cuda.device(env["dev"]):
        assert lib.rg_cell_overlap_i32(nat.ptr(lp), nat.ptr(pp), nat.ptr(ln), nat.ptr(pn), n, h, w, pairs, nat.ptr(rows),
                                       nat.ptr(count), nat.ptr(totals), nat.ptr(workspace), need, nat.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert totals.cpu().tolist() == [pairs, 0]
    r, c = rows.cpu().numpy(), count.cpu().numpy()
    assert (r[pairs:] == -77).all() and (c[pairs:] == -77).all()
    order = np.lexsort((r[:pairs, 1], r[:pairs, 0]))
    np.testing.assert_array_equal(r[:pairs, 0][order], want[0])
    np.testing.assert_array_equal(r[:pairs, 1][order], want[1])
    np.testing.assert_array_equal(c[:pairs][order], want[2])


# ---- index sums that pass 2^32 inside a wavefront's scan -----------------------------------------------------------------------
def test_index_sums_shuffled_between_lanes_pass_2_to_the_32(env):
    """One line of n = 2^27 + 2^21 pixels in two cells, cut inside a wavefront at m = 2^27 - 37, as a row (x carries the
    magnitude) and as a column (y does).  The segmented scan of ``cc_stats_kernel`` doubles its span every step, so the widest
    value that ever goes through ``shfl_up_i64`` is the 32-lane partial sum of step d = 32.  From coordinate 2^27 on -- 32 768
    wavefronts here -- that partial is 2^32 or more: the high half of the shuffle is not zero, and a wavefront's final sum is
    2^33 or more before the atomic add.  Labels, values and ``cell_ptr`` are made on the device; ``area`` and ``sum_yx`` come
    from ``rg_component_stats_f32`` with every other output NULL; the expected sums are Python integers."""
    torch, nat, lib, dev = env["torch"], env["native"], env["lib"], env["dev"]
    n, m = 2 ** 27 + 2 ** 21, 2 ** 27 - 37
    full = -(-m // 64) * 64                                      # the first wavefront that lies in the second cell alone
    assert 32 * full >= 2 ** 32 and full + 64 <= n < 2 ** 31     # its lanes 0 .. 31 sum to 2^32: what lane 63 takes at d = 32
    # 1.02 GiB of device memory for the two arrays below (4 bytes per pixel each), none on the host
    labels = torch.ones(n, dtype=torch.int32, device=dev)
    labels[m:] = 2
    src = torch.zeros(n, dtype=torch.float32, device=dev)
    cell_ptr = torch.tensor([0, 2], dtype=torch.int32, device=dev)
    sums = [m * (m - 1) // 2, n * (n - 1) // 2 - m * (m - 1) // 2]
    assert sums[1] < 2 ** 63
    for what, (h, w) in (("row", (1, n)), ("column", (n, 1))):
        area = torch.full((2,), -77, dtype=torch.int32, device=dev)
        sum_yx = torch.full((2, 2), -77, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            assert lib.rg_component_stats_f32(nat.ptr(src), nat.ptr(labels), nat.ptr(cell_ptr), 1, h, w, 2, nat.ptr(area), 0,
                                              nat.ptr(sum_yx), 0, 0, 0, nat.stream_ptr()) == 0
        torch.cuda.synchronize()
        want = [[0, v] if what == "row" else [v, 0] for v in sums]
        print(f"{what} of {n} pixels: sum_yx {sum_yx.cpu().tolist()}, expected {want}")
        assert area.cpu().tolist() == [m, n - m], what
        assert sum_yx.cpu().tolist() == want, what
