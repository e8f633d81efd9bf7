"""The scenes of tests/slab_scenes.py still hold what the slab-seam GPU tests rely on (no GPU needed): recomputed with the
oracle and with NumPy alone, so a run without a GPU proves that the fixtures have their seams, chunk kinds and rotations."""
import numpy as np

import slab_scenes as scenes
from conftest import golden_names, grid_spec, load_golden


def test_layout_constants_are_the_build_s():
    from radar_processor_amd import _native
    assert (scenes.LINES, scenes.ROTATION, scenes.DENSE_MAX) == (_native.RG_COMPACT_LINES, _native.RG_COMPACT_ROTATION,
                                                                _native.RG_DENSE_MAX_DICT)
    assert (scenes.ORDER_SEGMENT, scenes.ORDER_DISPATCH) == (_native.RG_REC_ORDER_SEGMENT, _native.RG_REC_ORDER_DISPATCH)


def test_wide_scene_has_its_chunk_kinds_and_seams():
    """53 912 pairs in levels of [47024, 4912, 1416, 460, 100, 0]; 54 chunks of three segments per line, 52 of them with at
    most 2048 gates (18 empty), two wider; a row of 1073 pairs; and the four slab sizes cut the levels as tabulated."""
    w = scenes.wide_scene()
    nsx, nyg, n_chunks = scenes.layout(scenes.WIDE_SHAPE)
    assert (nsx, nyg, n_chunks) == (3, 3, 54) and scenes.WIDE_SHAPE[1] % scenes.LINES == 2
    assert w["vol"].n_total_gates == 64800 and int(w["indptr"][-1]) == 53912
    assert list(w["level_pairs"]) == scenes.WIDE_LEVEL_PAIRS and w["level_pairs"][-1] == 0
    sizes = w["chunk_sizes"]
    dense, wide, empty = sizes <= scenes.DENSE_MAX, sizes > scenes.DENSE_MAX, sizes == 0
    assert int(dense.sum()) == 52 and sorted(sizes[wide]) == scenes.WIDE_WIDE_CHUNKS and int(empty.sum()) == scenes.WIDE_EMPTY_CHUNKS
    assert (dense & ~empty).any() and wide.any() and empty.any()
    assert np.array_equal(w["chunk_pairs"] == 0, empty)
    assert int(np.diff(w["indptr"]).max()) == scenes.WIDE_LONGEST_ROW
    print(f"wide scene: {int(dense.sum())} dense / {int(wide.sum())} wide / {int(empty.sum())} empty chunks")
    for cap, slabs in scenes.WIDE_SLABS.items():
        assert scenes.slabs_for(w["level_pairs"], cap) == slabs, cap
    # the weightings share the neighbour sets; Barnes and uniform weights fit the 26-bit code above exponent 120
    for name in ("barnes2", "nearest"):
        bits = w["w32"][name].view(np.uint32).astype(np.int64) - scenes.W_BASE
        assert bits.min() >= 0 and bits.max() <= scenes.CODE_MAX
    assert w["w32"]["cressman"].min() < 2.0 ** -7


def test_windowed_wide_scene_rotates_its_slabs_differently():
    """Three line groups and three segments give every level of the wide scene the same rotation; its first eight lines have
    two line groups, and the slabs that start at levels 1 and 2 -- both with pairs -- are rotated by one and two columns more
    than a grid of their own.  Dense and wide chunks remain, and a slab per level is still what one pair per slab gives."""
    nsx, nyg, _ = scenes.layout(scenes.WIDE_SHAPE)
    assert {scenes.rotation_of_group(p * nyg, nsx) for p in range(scenes.WIDE_SHAPE[0])} == {0}
    win = scenes.wide_window_scene()
    nsx, nyg, n_chunks = scenes.layout(scenes.WINDOW_SHAPE)
    assert (nsx, nyg, n_chunks) == (3, 2, 36)
    assert [scenes.rotation_of_group(p * nyg, nsx) for p in range(3)] == [0, 1, 2] and (win["level_pairs"][:3] > 1).all()
    sizes = win["chunk_sizes"]
    assert (sizes > scenes.DENSE_MAX).any() and ((sizes > 0) & (sizes <= scenes.DENSE_MAX)).any() and (sizes == 0).any()
    assert scenes.slabs_for(win["level_pairs"], 1) == scenes.WIDE_SLABS[1]
    whole = scenes.wide_scene()
    assert 0 < int(win["indptr"][-1]) < int(whole["indptr"][-1]) and win["idx"].size == win["w32"]["barnes2"].size
    assert np.array_equal(win["indptr"][:150 * 8 + 1], whole["indptr"][:150 * 8 + 1])     # level 0, lines 0 .. 7: the same rows


def test_hand_made_slab_case_holds_what_it_promises():
    """At least 5 planes, a ragged last line group, three segments per line, every residue of the extra rotation over the
    planes, dictionaries of exactly 2048 and 2049 entries with their last entry in use, a plane and a segment without
    pairs, rows of at least 400 pairs -- and later slabs start at a row pointer other than 0."""
    c = scenes.make_slab_case()
    nz, ny, nx = c["shape"]
    nsx, nyg, n_chunks = scenes.layout(c["shape"])
    assert nz >= 5 and ny % scenes.LINES and (nsx, nyg) == (3, 2) and scenes.segment_starts(nx) == [0, 44, 87, 130]
    assert {scenes.rotation_of_group(plane0 * nyg, nsx) for plane0 in range(nz)} == set(range(nsx))
    sizes, level_ptr = c["sizes"], c["indptr"][::ny * nx]
    assert scenes.DENSE_MAX in sizes and scenes.DENSE_MAX + 1 in sizes
    for c_id in np.nonzero(sizes)[0]:
        assert c["pos"][c["chunk_of_pair"] == c_id].max() == sizes[c_id] - 1
    pairs = np.diff(level_ptr)
    assert pairs[scenes.SLAB_EMPTY_PLANE] == 0 and (np.delete(pairs, scenes.SLAB_EMPTY_PLANE) > 0).all() and level_ptr[1] > 0
    seg_pairs = [int(c["indptr"][r0 + n] - c["indptr"][r0]) for (_, _, r0, n, _) in scenes.segments(c["shape"])]
    assert seg_pairs[1 * nsx + 1] == 0 and c["lengths"].max() >= 400 and {0, 1, 2, 3, 4} <= set(np.unique(c["lengths"]))
    for parts in scenes.SLAB_PARTITIONS:
        assert parts[0][0] == 0 and parts[-1][1] == nz and all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
    assert any((p0, p1) == (scenes.SLAB_EMPTY_PLANE, scenes.SLAB_EMPTY_PLANE + 1) for parts in scenes.SLAB_PARTITIONS
               for (p0, p1) in parts)
    # every segment has a slot of its own in the whole grid's dispatch order ...
    whole, n_slots = scenes.slot_table(c["shape"], scenes.ORDER_DISPATCH)
    assert sorted(whole.values()) == sorted(set(whole.values())) and len(whole) == nz * ny * nsx
    # ... and a slab that starts at plane0 has the whole grid's slots shifted by its first slot only when its rotation counts
    # the line groups in front of it: a one-plane grid's own table, rotated by plane0's groups, against the whole table
    per_plane = n_slots // nz
    for plane0 in range(nz):
        extra = scenes.rotation_of_group(plane0 * nyg, nsx)
        own, _ = scenes.slot_table((1, ny, nx), scenes.ORDER_DISPATCH)
        for (y, sx), slot in own.items():
            block, wave = divmod(slot, scenes.LINES)
            grp, col = divmod(block, nsx)
            # the slab's block that reads segment sx of its group sits ``extra`` columns further back in the whole grid
            moved = (grp * nsx + (col - extra) % nsx) * scenes.LINES + wave
            assert whole[(plane0 * ny + y, sx)] == plane0 * per_plane + moved, (plane0, y, sx)


def test_reference_fixtures_have_a_level_seam_to_cut_at():
    """Every g3 / g4 / g6 fixture with pairs has an interior level i at which ``pairs_per_slab = L[i] + L[i+1]`` fills a slab
    exactly and one pair less cuts it elsewhere; levels without pairs exist at the start, the end and in the middle."""
    seen = set()
    for name in golden_names("g3_") + golden_names("g4_") + golden_names("g6_"):
        meta, ref = load_golden(name)
        shape, _ = grid_spec(meta)
        level_pairs = np.diff(ref["indptr"][::shape[1] * shape[2]].astype(np.int64))
        if level_pairs.sum() == 0:
            assert name == "g3_c2_corner_barnes2"
            continue
        assert scenes.seam_level(level_pairs) is not None, name
        live = np.nonzero(level_pairs)[0]
        seen |= {"leading"} if live[0] > 0 else set()
        seen |= {"trailing"} if live[-1] < shape[0] - 1 else set()
        seen |= {"interior"} if (level_pairs[live[0]:live[-1]] == 0).any() else set()
    assert seen == {"leading", "trailing", "interior"}
