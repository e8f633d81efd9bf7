"""The pairs of tests/graph_replay_scenes.py can catch what the replay tests are for -- proved on the CPU, since no broken
build is ever run on the device.  A replay that reproduced A's result, a key left in the overlap table, or an output that
never changes would each be invisible with a careless pair; these conditions rule that out."""
import numpy as np
import pytest

import graph_replay_scenes as gs

LARGE = 64                         # outputs with more elements than this must differ in at least 1 % of them
SHARE = 0.01


def _rows(a):
    return {tuple(r) for r in np.asarray(a).reshape(len(a), -1).tolist()}


def _differing_share(chain, key, a, b):
    """The share of B's elements (rows, for an unordered output) that A does not hold in the same place."""
    if key in gs.UNORDERED.get(chain, ()):
        rows_a, rows_b = _rows(a), _rows(b)
        return len(rows_b - rows_a) / max(len(rows_b), 1)
    extra = 0
    if key in gs.PER_CELL.get(chain, ()):                                     # rows beyond the shorter table all differ
        rows = min(len(a), len(b))
        extra, a, b = len(b) - rows, a[:rows], b[:rows]
    assert a.shape == b.shape and a.dtype == b.dtype, (chain, key)
    same = (a == b) | ((a != a) & (b != b)) if a.dtype.kind == "f" else a == b
    per_row = same.size // max(len(same), 1)
    return 1.0 - float(same.sum()) / float(same.size + extra * per_row)


def _inputs(chain, which):
    s = getattr(gs, chain)(which)
    values = s.values() if isinstance(s, dict) else s
    return [a for a in values if isinstance(a, np.ndarray)]


@pytest.mark.parametrize("chain", gs.CHAINS)
def test_a_and_b_have_the_same_shapes_and_dtypes_and_differ(chain):
    a, b = _inputs(chain, "A"), _inputs(chain, "B")
    assert len(a) == len(b) and len(a) >= 1
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype, chain
    assert any(x.tobytes() != y.tobytes() for x, y in zip(a, b))
    ea, eb = gs.expected(chain, "A"), gs.expected(chain, "B")
    assert list(ea) == list(eb)
    for key in ea:
        if key not in gs.UNORDERED.get(chain, ()) + gs.PER_CELL.get(chain, ()):
            assert ea[key].shape == eb[key].shape and ea[key].dtype == eb[key].dtype, (chain, key)


def test_the_host_side_parameters_of_a_and_b_are_the_same():
    a, b = gs.verification("A"), gs.verification("B")
    assert a.thresholds == b.thresholds and a.scales == b.scales and (a.mask is None) == (b.mask is None)
    a, b = gs.convection("A"), gs.convection("B")
    assert a[3:] == b[3:]                                                       # footprints, edges and scalars
    a, b = gs.motion("A"), gs.motion("B")
    assert (a.B, a.S, a.R, a.min_echo) == (b.B, b.S, b.R, b.min_echo) and a.mask_prev is None and b.mask_prev is None
    assert tuple(gs.motion_field("A")[1]) == tuple(gs.motion_field("B")[1])
    a, b = gs.accumulation("A"), gs.accumulation("B")
    assert a.bilinear is b.bilinear and a.nearest is b.nearest


@pytest.mark.parametrize("chain", gs.CHAINS)
def test_b_differs_from_a_in_every_output(chain):
    ea, eb = gs.expected(chain, "A"), gs.expected(chain, "B")
    for key in ea:
        share = _differing_share(chain, key, ea[key], eb[key])
        print(f"{chain} / {key}: {eb[key].size} elements, {100.0 * share:.1f} % differ")
        if key in gs.GEOMETRY_ONLY.get(chain, ()):
            assert share == 0.0, f"{chain} / {key} is listed as following from the host-side parameters alone"
            continue
        assert share > 0.0, f"{chain} / {key}: a replay that reproduced A's result would pass"
        if eb[key].size > LARGE:
            assert share >= SHARE, f"{chain} / {key}: only {100.0 * share:.2f} % of the elements differ"


@pytest.mark.parametrize("chain", gs.CHAINS)
@pytest.mark.parametrize("which", gs.WHICH)
def test_no_output_is_trivial(chain, which):
    """Not one value throughout (all zero, all fill, all NaN), so poison that survives cannot pass for a result."""
    for key, a in gs.expected(chain, which).items():
        if key in gs.MAY_BE_TRIVIAL.get(chain, ()):
            continue
        first = a.reshape(-1)[:1]
        assert a.size > 1 and (a.view(np.uint8).reshape(a.size, -1) != first.view(np.uint8)).any(), (chain, which, key)
        if a.dtype.kind == "f":
            assert np.isfinite(a).any(), (chain, which, key)
        assert np.count_nonzero(a) > 0, (chain, which, key)


def test_the_cell_overlap_table_is_dirtied():
    """B's pairs occupy slots that A's do not and the other way round: a key that the call failed to clear would come out as
    a pair of the wrong scene."""
    pairs = {w: gs.expected("tracking", w)["pairs"] for w in gs.WHICH}
    for w in gs.WHICH:
        assert 0 < len(pairs[w]) <= gs.TRACK_MAX_PAIRS                          # the explicit max_pairs holds both scenes
        s = gs.tracking(w)
        assert max(int(s.ptr_prev[-1]), int(s.ptr_next[-1])) <= gs.TRACK_CELLS
    slots = {w: gs.overlap_slots(pairs[w], gs.TRACK_MAX_PAIRS) for w in gs.WHICH}
    capacity = gs.overlap_capacity(gs.TRACK_MAX_PAIRS)
    assert capacity == 256 and all(len(slots[w]) == len(pairs[w]) and max(slots[w]) < capacity for w in gs.WHICH)
    only_a, only_b = slots["A"] - slots["B"], slots["B"] - slots["A"]
    print(f"{len(slots['A'])} and {len(slots['B'])} slots of {capacity}; {len(only_a)} only A's, {len(only_b)} only B's")
    assert len(only_a) >= 8 and len(only_b) >= 8
    assert _rows(pairs["B"]) - _rows(pairs["A"]) and _rows(pairs["A"]) - _rows(pairs["B"])


def test_the_slot_function_is_the_finaliser_of_splitmix64():
    """Known answers of the restated slot function: the first outputs of splitmix64 are its finaliser applied to multiples of
    the golden-ratio increment (Steele, Lea and Flood 2014; the reference values of Vigna's splitmix64.c for seed 0)."""
    gamma, capacity = 0x9E3779B97F4A7C15, 1 << 64
    want = (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F)
    for k, value in enumerate(want, start=1):
        key = gamma * k % capacity
        assert gs.overlap_home_slot(key >> 32, key & 0xFFFFFFFF, capacity) == value


def test_the_in_place_relabel_has_something_to_restore():
    """rg_relabel_cells_i32 runs in place on labels_next: its result must differ from its input, or a replay on the result of
    the replay before would pass without the input restored."""
    for w in gs.WHICH:
        s = gs.tracking(w)
        assert (gs.expected("tracking", w)["relabel_next"] != s.labels_next).mean() >= SHARE


def test_the_components_workspace_is_dirtied():
    """A and B differ in the number of cells of each plane and in the tiles that hold foreground, so the parents, the chunk
    counts and the running cell counts A leaves in the workspace are wrong for B wherever they are read before written."""
    ptr = {w: gs.cells_reference(w)[1] for w in gs.WHICH}
    per_plane = {w: np.diff(ptr[w]) for w in gs.WHICH}
    print(f"cells per plane: A {per_plane['A'].tolist()}, B {per_plane['B'].tolist()}")
    assert (per_plane["A"] != per_plane["B"]).all() and (per_plane["A"] > 0).all() and (per_plane["B"] > 0).all()
    assert max(int(ptr["A"][-1]), int(ptr["B"][-1])) <= gs.CELLS_BOUND
    tiles = {w: gs.tiles_with_foreground(w) for w in gs.WHICH}
    assert tiles["A"] - tiles["B"] and tiles["B"] - tiles["A"]
    for w in gs.WHICH:                                                          # the despeckling removes some cells and keeps others
        removed, labels = gs.expected("cells", w)["removed"], gs.cells_reference(w)[0]
        assert 0 < removed.sum() < (labels > 0).sum() and gs.cells(w).mask.any()
