"""CPU-side checks of tests/cell_scale_scenes.py (no GPU needed): each scene reaches the path it was built for.  These are
conditions on the scenes, not measurements: more than one trip of ``cc_scan_kernel``, a trip boundary inside a plane, index
sums above 2^32, cell counts far above one workgroup -- so a changed kernel constant fails here, loudly, and does not silently
shrink what tests/test_gpu_cell_scale.py covers."""
import time

import numpy as np

import cell_scale_scenes as css
import components_oracle as co
import radar_processor_amd as rg
import tracking_oracle as to
from radar_processor_amd import _native


def _cells(name, connectivity):
    return int(css.labelled(name, connectivity)[1][-1])


def test_the_whole_module_builds_in_a_few_seconds():
    """Scenes and oracle labellings of every case: what the GPU file pays before its first launch.  First in the file, so
    that the caches are cold when the whole file runs; a guard against a scene that became slow, not a measurement."""
    start = time.perf_counter()
    css.scenes()
    built = time.perf_counter() - start
    for name, connectivity in css.CASES:
        css.labelled(name, connectivity)
    css.overlap_scenes()
    total = time.perf_counter() - start
    print(f"scenes {built:.2f} s, with every labelling {total:.2f} s")
    assert total < 30.0


def test_kernel_constants_were_found_in_the_sources():
    assert css.BLOCK is not None, "kBlock not found in csrc/rg_common.hpp"
    assert css.PER_THREAD is not None, "kPerThread not found in csrc/rg_components.hip"
    assert css.BLOCK > 0 and css.PER_THREAD > 0 and css.CHUNK == css.BLOCK * css.PER_THREAD
    assert (css.TH, css.TW) == (_native.RG_CC_TILE_H, _native.RG_CC_TILE_W)
    # the shapes the module's docstring states, with the constants as they are today
    if (css.TH, css.TW, css.BLOCK, css.PER_THREAD) == (32, 64, 256, 4):
        assert css.MANY_PLANES == 600 and css.STRADDLE_SHAPE == (33, 65) and css.BIG == (520, 517)


def test_every_stack_takes_more_than_one_scan_trip():
    for name, trips in (("many_planes", 3), ("many_planes_wrap", 3), ("straddle", 2), ("random_0.41", 2)):
        shape3 = css.scene(name).planes.shape
        print(f"{name}: {shape3}, {css.chunks_of(shape3)} chunks, {css.scan_trips(shape3)} scan trips")
        assert css.chunks_of(shape3) > css.BLOCK and css.scan_trips(shape3) >= trips
    assert all(css.scene(name).planes.shape == (1,) + css.BIG for name, _ in css.BIG_CASES)
    # one chunk per plane: every trip writes cell_ptr entries; a wavefront holds several plane boundaries
    n, h, w = css.scene("many_planes").planes.shape
    assert h * w <= css.CHUNK and css.chunks_of((n, h, w)) == n and 64 // (h * w) >= 8
    # the big plane: many tiles, ragged both ways, a ragged last chunk
    h, w = css.BIG
    assert h % css.TH and w % css.TW and (h * w) % css.CHUNK and -(-h // css.TH) * -(-w // css.TW) > 128


def test_the_trip_boundary_of_straddle_falls_inside_a_plane():
    n, h, w = css.scene("straddle").planes.shape
    per_plane = -(-h * w // css.CHUNK)
    assert per_plane >= 3 and n * per_plane > css.BLOCK
    assert 0 < css.BLOCK % per_plane < per_plane - 1                     # chunk 256: not a plane's first chunk, not its last
    plane = css.BLOCK // per_plane
    ptr = css.labelled("straddle", 8)[1]
    assert ptr[plane + 1] > ptr[plane] and plane + 1 < n                 # that plane has cells, and planes follow it
    assert -(-h // css.TH) == 2 and -(-w // css.TW) == 2                 # four tiles: both seam kinds


def test_many_planes_has_empty_planes_and_label_1_on_both_sides_of_most_boundaries():
    s = css.scene("many_planes")
    fg = co.foreground(s.planes, s.lo)
    assert fg[0].all() and fg[-1].all() and not fg[7].any() and not fg[595].any()
    assert css.scene("many_planes_wrap").planes.tobytes() == s.planes.tobytes() and css.scene("many_planes_wrap").wrap
    for connectivity in (4, 8):
        labels, ptr = css.labelled("many_planes", connectivity)
        last, first = labels[:-1].reshape(len(labels) - 1, -1)[:, -1], labels[1:].reshape(len(labels) - 1, -1)[:, 0]
        both = int(((last > 0) & (last == first)).sum())
        print(f"many_planes connectivity {connectivity}: {int(ptr[-1])} cells, {both} boundaries with equal labels on both sides")
        assert both > 60 and (np.diff(ptr) == 0).sum() >= 85 and np.diff(ptr).max() >= 2
    # the second stack of the overlap test differs, and has equal labels across boundaries too
    other = css.overlap_scene("many_planes")
    assert other.labels_next.shape == other.labels_prev.shape and (other.labels_next != other.labels_prev).any()


def test_long_lines_have_index_sums_above_2_to_the_32():
    for name in ("long_row", "long_row_cut", "long_column", "long_column_cut", "long_column_cut_wrap"):
        labels, ptr, table = css.line_expected(name)
        print(f"{name}: {int(ptr[-1])} cells, areas {table['area'].tolist()}, sum_yx {table['sum_yx'].tolist()}")
        # a line in one cell sums to 4 999 950 000 (less the cut pixel): bit 32 is set.  The two cells of a line cut at
        # 70 001 split that sum almost evenly: neither can reach 2^32, both set bit 31 of the low word
        if name in ("long_row", "long_column", "long_column_cut_wrap"):
            assert len(table["area"]) == 1 and int(table["sum_yx"].max()) >= 2 ** 32, name
        else:
            assert name in ("long_row_cut", "long_column_cut") and len(table["area"]) == 2
            assert 2 ** 31 <= int(table["sum_yx"].max(axis=1).min()) and int(table["sum_yx"].max()) < 2 ** 32, name
        assert int(table["area"].sum()) == css.LINE - ("cut" in name)
    whole = css.line_expected("long_row")[2]
    assert whole["sum_yx"].tolist() == [[0, 4_999_950_000]] and whole["bbox"].tolist() == [[0, 0, 0, css.LINE - 1]]
    assert css.line_expected("long_column")[2]["sum_yx"].tolist() == [[4_999_950_000, 0]]
    # the maximum sits at the last pixel and at earlier ones: argmax is the earliest of the cell
    assert whole["argmax"].tolist() == [css.PEAKS[0]] and whole["vmax"].tolist() == [css.PEAK]
    assert css.scene("long_row").planes.ravel()[-1] == css.PEAK
    assert css.line_expected("long_row_cut")[2]["argmax"].tolist() == [css.PEAKS[0], css.PEAKS[2]]
    assert css.line_expected("long_column_cut_wrap")[2]["argmax"].tolist() == [css.PEAKS[0]]
    # more tiles than any other scene, side by side and on top of each other
    assert css.LINE // css.TW > 1500 and css.LINE // css.TH > 3000


def test_the_closed_forms_of_the_lines_are_what_the_oracle_computes():
    """The flood fill and ``co.stats`` on the lines themselves: the closed forms the GPU tests compare against are right.  The
    cut column is one cell under wrap_rows and two without."""
    for name, connectivity in (("long_row", 4), ("long_row_cut", 8), ("long_column_cut", 4), ("long_column_cut_wrap", 8)):
        s = css.scene(name)
        labels, ptr, table = css.line_expected(name)
        got_labels, got_ptr = co.label(s.planes, s.lo, s.hi, s.mask, connectivity, s.wrap)
        np.testing.assert_array_equal(got_ptr, ptr, err_msg=name)
        np.testing.assert_array_equal(got_labels, labels, err_msg=name)
        want = co.stats(s.planes, got_labels, got_ptr)
        assert sorted(want) == sorted(table)
        for key, column in want.items():
            assert column.dtype == table[key].dtype and column.tobytes() == table[key].tobytes(), (name, key)
    assert css.line_expected("long_column_cut_wrap")[1].tolist() == [0, 1]
    assert css.line_expected("long_column_cut")[1].tolist() == [0, 2]
    row = css.scene("long_row_cut")                                      # wrap_rows joins nothing in a plane of one row
    assert co.label(row.planes, row.lo, connectivity=8, wrap_rows=True)[1].tolist() == [0, 2]


def test_the_patterns_of_the_big_plane_are_what_they_are_for():
    h, w = css.BIG
    assert _cells("serpentine", 4) == 1 and _cells("comb", 8) == 1 and _cells("all_foreground", 8) == 1
    assert _cells("wrap_serpentine", 4) == 1
    assert _cells("checkerboard", 4) == (h * w + 1) // 2 > 65536
    serpentine = co.foreground(css.scene("serpentine").planes, css.LO)
    assert int(serpentine.sum()) > h * w // 2 - w
    for name, connectivity in (("random_0.41", 8), ("random_0.593", 4), ("wrap_random_0.45", 8)):
        labels, ptr = css.labelled(name, connectivity)
        area = np.bincount(labels.ravel())[1:]
        biggest = labels[0] == int(area.argmax()) + 1
        tiles = {(y // css.TH, x // css.TW) for y, x in zip(*np.nonzero(biggest))}
        print(f"{name} connectivity {connectivity}: {int(ptr[-1])} cells, largest {int(area.max())} pixels in {len(tiles)} tiles")
        assert int(ptr[-1]) > 1000 and len(tiles) > 16                   # at the threshold: a cell that wanders through tiles
    # the wrap joins cells: fewer of them than without
    s = css.scene("wrap_random_0.45")
    assert _cells("wrap_random_0.45", 8) < int(co.label(s.planes, s.lo, connectivity=8)[1][-1])


def test_the_vectorised_table_equals_the_oracle_table():
    """``vector_table`` against ``co.stats`` where both are affordable: many planes, and many cells of every size."""
    for name, connectivity in (("many_planes", 8), ("straddle", 4), ("random_0.41", 8)):
        s = css.scene(name)
        labels, ptr = css.labelled(name, connectivity)
        want, got = co.stats(s.planes, labels, ptr), css.vector_table(s.planes, labels, ptr)
        for key, column in got.items():
            assert column.dtype == want[key].dtype and column.tobytes() == want[key].tobytes(), (name, key)


def test_overlap_scenes_hold_the_pairs_they_are_for():
    h, w = css.BIG
    pairs = {name: to.overlap(*css.overlap_scene(name)[1:]) for name in css.OVERLAP_NAMES}
    for name, (a, b, c) in pairs.items():
        print(f"{name}: {len(c)} pairs, largest {int(c.max())} pixels")
    a, b, c = pairs["checker_vs_all"]
    assert len(c) == (h * w + 1) // 2 and (b == 0).all() and (c == 1).all() and (a == np.arange(len(c))).all()
    # the default max_pairs is min(pixels, cells_prev * cells_next) = the pair count here; the library sizes the table for it
    # (12 bytes per slot, asked on the host): at most half full
    lib = rg.load_library(require_device=False)
    scene = css.overlap_scene("checker_vs_all")
    default = min(h * w, int(scene.ptr_prev[-1]) * int(scene.ptr_next[-1]))
    slots = int(lib.rg_cell_overlap_workspace_bytes(default)) // 12
    assert default == len(c)
    assert slots > 0 and 2 * len(c) <= slots
    a, b, c = pairs["long_row_vs_cut"]
    assert a.tolist() == [0, 0] and b.tolist() == [0, 1] and c.tolist() == [css.CUT, css.LINE - css.CUT - 1]
    assert min(c) // 64 > 400                                            # each pair is fed by hundreds of wavefronts
    assert len(pairs["many_planes"][2]) > 300 and len(pairs["random_0.41_shifted"][2]) > 1000
