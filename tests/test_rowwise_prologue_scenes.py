"""What ``rowwise_prologue_scenes`` promises (no GPU), and the row-wise kernel's pair test against its definition."""
import numpy as np
import pytest

import rowwise_prologue_scenes as scenes


def test_constants_are_the_librarys():
    from radar_processor_amd import _native
    assert (scenes.LINES, scenes.ROTATION) == (_native.RG_COMPACT_LINES, _native.RG_COMPACT_ROTATION)
    assert scenes.N_GATES <= _native.RG_DENSE_MAX_DICT


def test_grid_is_cut_as_described():
    segs = scenes.segments()
    nz, ny, nx = scenes.SHAPE
    assert (nz, ny, nx) == (2, 5, 70) and len(segs) == nz * ny * 2 and all(s[3] == 35 for s in segs)
    assert sorted({s[4] for s in segs}) == list(range(8))
    # the second line group of a plane is line 4 alone: three of its workgroup's four wavefronts have no rows
    for chunk in range(8):
        lines = sorted({s[0] % ny for s in segs if s[4] == chunk})
        assert lines == ([0, 1, 2, 3] if (chunk // 2) % 2 == 0 else [4])
    order = scenes.dispatch_chunks()
    assert sorted(order) == list(range(8)) and order[0] == 0 and order[-1] == 6
    from radar_processor_amd.grid_geometry import CompactCSR
    from radar_processor_amd import _native
    for (line, sx, r0, nrows, chunk) in segs:       # the library's own restatement of the dispatch order
        slot = int(CompactCSR.slot_of_segments(np.array([line]), np.array([sx]), scenes.SHAPE, _native.RG_REC_ORDER_DISPATCH)[0])
        assert order[slot // scenes.LINES] == chunk and slot % scenes.LINES == (line % ny) % scenes.LINES


@pytest.mark.parametrize("variant", scenes.VARIANTS)
def test_scene_holds_what_it_promises(variant):
    c = scenes.scene(variant)
    nz, ny, nx = c["shape"]
    ip, lengths, pairs = c["indptr"], c["lengths"], c["chunk_pairs"]
    order = scenes.dispatch_chunks()
    assert pairs[order[0]] == 0                                            # the first chunk has none
    assert (pairs[order[-1]] > 0) == (variant == "full")                   # the last one: with and without
    assert (pairs[7] > 0) == (variant == "full")                           # ... and the chunk that reads dict_ptr's last entry
    assert 250 <= c["n_gates"] <= 350 and len(np.unique(c["gidx"])) > 200 and int(c["gidx"].max()) < c["n_gates"]
    assert float(c["wts"].min()) >= 0.02 and float(c["wts"].max()) <= 1.0
    # one chunk has pairs in its fourth line only
    per_line = {}
    for (line, sx, r0, nrows, chunk) in scenes.segments():
        per_line.setdefault(chunk, {})[line % ny] = int(ip[r0 + nrows] - ip[r0])
    assert [per_line[1][y] > 0 for y in range(4)] == [False, False, False, True]
    # a whole plane without a pair (variant "empty")
    plane_pairs = [int(ip[(p + 1) * ny * nx] - ip[p * ny * nx]) for p in range(nz)]
    assert plane_pairs[0] > 0 and (plane_pairs[1] == 0) == (variant == "empty")
    assert set(np.unique(lengths)) == set(scenes.LENGTHS)
    starts, ends, populated = set(), set(), 0
    for (line, sx, r0, nrows, chunk) in scenes.segments():
        span = int(ip[r0 + nrows] - ip[r0])
        if span == 0:
            continue
        populated += 1
        assert span <= 65534                                              # every segment on the 16-bit row ends
        seg = lengths[r0:r0 + nrows]
        assert tuple(seg[:len(scenes.HEAD)]) == scenes.HEAD and seg[nrows - 1] == 0
        rel = ip[r0:r0 + nrows + 1] - ip[r0]
        live = seg > 0
        starts |= {int(v) % 3 for v in rel[:-1][live]}
        ends |= {int(v) % 3 for v in rel[1:][live]}
        # three one-pair rows share record 0, empty rows before, between and behind them
        ones = [r for r in range(6) if seg[r] == 1]
        assert ones == [1, 3, 4] and {int(rel[r]) // 3 for r in ones} == {0} and seg[0] == seg[2] == seg[5] == 0
        # the long row takes several steps of three records at one lane per row
        long_row = int(np.argmax(seg))
        n_rec = (int(rel[long_row + 1]) + 2) // 3 - int(rel[long_row]) // 3
        assert seg[long_row] == 200 and n_rec >= 4 * 3
    assert starts == {0, 1, 2} and ends == {0, 1, 2}
    assert populated == (1 + 2 + 10 if variant == "full" else 1 + 2)
    f = c["fields"]
    assert any(np.isnan(x).any() for x in f) and any(np.isposinf(x).any() for x in f) and any(np.isneginf(x).any() for x in f)
    assert any((x < 0).any() for x in f) and sum(m is not None and m.any() for m in c["masks"]) >= 2
    # the special values are mentioned by pairs, and not all of them hidden by a mask
    used = np.zeros(c["n_gates"], dtype=bool)
    used[c["gidx"]] = True
    assert (used & ~np.isfinite(f[0]) & ~c["masks"][0]).any() and (used & ~np.isfinite(f[1])).any()


def test_pair_test_equals_its_definition():
    """The kernel's test -- ``3 k L + i < lo0 + len`` and, for pairs 0 and 1 of slot 0, ``lo0 <= i`` -- against the definition
    (the slot holds a record of the row, and the pair's number lies in the row), exhaustively over the first pair's residue,
    the row's length, lanes per row, lane, steps advanced, slot and pair; a lane without a row (dead in its round) as well."""
    checked = mine = 0
    for qs in (0, 1, 2, 3, 4, 5, 598, 599, 600):
        for length in list(range(13)) + [200]:
            for lanes in (1, 2, 8, 64):
                for sub in range(lanes):
                    for steps in range(4):
                        for live in (True, False):
                            lo0, ln, q, q1 = scenes.step_state(qs, length, lanes, sub, steps, live=live)
                            if steps == 0:
                                assert lo0 <= 2
                            for k in range(3):
                                for i in range(3):
                                    want = scenes.pair_is_mine_definition(qs, length, q, q1, lanes, k, i, live=live)
                                    got = scenes.pair_is_mine_kernel(lo0, ln, lanes, k, i)
                                    assert got == want, (qs, length, lanes, sub, steps, live, k, i)
                                    checked += 1
                                    mine += want
    assert checked > 300_000 and mine > 1000
    # every pair of a row is taken by exactly one (lane, step, slot, pair)
    for qs, length, lanes in ((0, 200, 1), (1, 200, 2), (2, 200, 8), (599, 12, 1), (598, 5, 64)):
        taken = []
        for sub in range(lanes):
            for steps in range(30):
                lo0, ln, q, q1 = scenes.step_state(qs, length, lanes, sub, steps)
                taken += [3 * (q + k * lanes) + i for k in range(3) for i in range(3)
                          if scenes.pair_is_mine_kernel(lo0, ln, lanes, k, i)]
        assert sorted(taken) == list(range(qs, qs + length)), (qs, length, lanes)
