"""``radar_processor_amd.pass_policy`` on the CPU: every decision against a frozen restatement of the code it was gathered
from, the memory thresholds at their edges, and what the decisions ask of the expensive things (the compact copy, its
records, the driver's free memory) and when.

The restatement (``parent_*`` below) is the commit before ``pass_policy`` existed, written down as straight-line code with
its own literals: ``CsrGridder.__init__`` and ``CsrGridder.apply`` (gridding.py), ``_use_compact``, ``_fields_per_pass``,
``volumes_per_pass_cap``, ``grid_products_device``'s ``run_fused`` (plane_products.py), ``CompactCSR.entry_bytes`` /
``window_for`` (grid_geometry.py).  It is not to be "fixed" together with the module: a decision that changes has to change
here too, on purpose (the precedent is ``SIGNATURES`` in test_mosaic_routes.py).
"""
import itertools
import os
import subprocess
import sys

import pytest

from radar_processor_amd import pass_policy as pp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GIB = 1 << 30
LAYOUTS = ("csr", "compact", "packed")      # full CSR; no gate_indices; no gate_indices and no weights


class Copy:
    """A compact copy that records what it is asked."""

    def __init__(self, window_cap=768, share=0.0, codable=True):
        self.window_cap, self.share, self.codable = window_cap, share, codable
        self.calls = []

    def fallback_fraction(self, window):
        self.calls.append(("fallback_fraction", window))
        return self.share

    def ensure_packed(self):
        self.calls.append("ensure_packed")
        return self.codable


class Source:
    """``copy_of``: yields ``copy`` (or ``None``) and counts the calls."""

    def __init__(self, copy):
        self.copy, self.asked = copy, 0

    def __call__(self):
        self.asked += 1
        return self.copy


# ---- the frozen restatement --------------------------------------------------------------------------------------------------
def parent_entry_bytes(n_fields, rowwise=False):
    if rowwise and n_fields >= 3:
        return 16 if n_fields == 3 else 20 if n_fields == 4 else 40
    if n_fields > 4:
        return 32
    return 4 * (2 if n_fields <= 2 else 3 if n_fields == 3 else 4)


def parent_window_for(window_cap, n_fields, lds_budget_bytes=None, rowwise=False):
    if lds_budget_bytes is None:
        lds_budget_bytes = 49152 if (rowwise and n_fields >= 3) else 32768
    room = max(0, lds_budget_bytes // parent_entry_bytes(n_fields, rowwise)) // 64 * 64
    return int(min(window_cap, room))


def parent_gridder(layout, n_pairs, device_compact, n_fields, compact, packed):
    """``CsrGridder.__init__`` -> ``(compact copy or None, window, packed_stream)``."""
    compact_only = layout != "csr"              # csr.gate_indices is None
    packed_only = layout == "packed"            # csr.weights is None
    want = compact or compact_only
    c = device_compact() if (want and n_pairs) else None
    window = 0
    packed_stream = False
    if c is not None:
        window = parent_window_for(c.window_cap, n_fields)
        if not compact_only and c.fallback_fraction(window) > 0.02:
            c, window = None, 0
    if c is not None:
        packed_stream = bool((packed or packed_only) and c.ensure_packed())
        if packed_stream:
            window = parent_window_for(c.window_cap, n_fields, rowwise=True)
        if not packed_stream and not compact_only and window * parent_entry_bytes(n_fields) > 24576:
            c, window = None, 0
    return c, window, packed_stream


def parent_apply(tile, packed_stream, has_compact, layout):
    """``CsrGridder.apply`` -> ``(entry point, its tile argument)``."""
    weights_none = layout == "packed"
    if has_compact and packed_stream and (tile in (0, 384) or tile >= 2000 or weights_none):
        return "rg_csr_compact_apply_packed_f32", tile if (tile == 384 or tile >= 2000) else 0
    if has_compact:
        return "rg_csr_compact_apply_f32", tile if tile in (128, 192, 256, 320, 384, 512) else 0
    return "rg_csr_apply_f32", tile if tile in (128, 192, 256, 320, 384, 512) else 0


def parent_use_compact(cached, n_pairs, mem_get_info):
    """``_use_compact``; ``cached``: ``None`` (nothing cached for this device CSR) or whether the cached copy is one."""
    if cached is not None:
        return cached
    if n_pairs < 50_000_000:
        return False
    free_b = mem_get_info()
    return free_b > 3.2 * n_pairs + (8 << 30)


def parent_fields_per_pass(layout, n_pairs, device_compact, use_compact):
    compact = None
    if layout == "packed":
        compact = device_compact()
    elif use_compact and n_pairs:
        compact = device_compact()
        if compact is not None and not compact.ensure_packed():
            compact = None
    if compact is not None:
        return 8 if compact.window_cap * parent_entry_bytes(8, rowwise=True) <= 32768 else 4
    return 8


def parent_volumes_per_pass_cap(layout, n_pairs, device_compact, use_compact):
    if layout == "packed" or (use_compact and n_pairs and device_compact() is not None and device_compact().ensure_packed()):
        return parent_fields_per_pass(layout, n_pairs, device_compact, use_compact)
    return min(4, 8)


def parent_run_fused(compact_is_none, packed_stream, n_fields, profile, nf, fused):
    has_columns_kernel = (not compact_is_none) and packed_stream and n_fields <= 4
    return bool(has_columns_kernel and not profile and (nf >= 5 if fused is None else bool(fused)))


# ---- the module against it ---------------------------------------------------------------------------------------------------
N_PAIRS = (0, 1, 49_999_999, 50_000_000)
SHARES = (0.0, 0.02, 0.0201)
WINDOW_CAPS = (256, 768, 1792, 4096, 8192)
TILES = (0, 128, 384, 512, 2004, 2075)


def test_window_arithmetic_is_the_parents():
    for nf, rowwise in itertools.product(range(1, 9), (False, True)):
        assert pp.entry_bytes(nf, rowwise) == parent_entry_bytes(nf, rowwise)
        for cap, budget in itertools.product(WINDOW_CAPS + (0, 64, 1216, 2432), (None, 0, 1000, 32768, 49152, 65536)):
            assert pp.window_for(cap, nf, rowwise, budget) == parent_window_for(cap, nf, budget, rowwise), (nf, rowwise, cap, budget)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_decision_of_a_pass_is_the_parents(layout):
    """The whole cross product of the discrete facts: the choice (copy used, window, records streamed, kernel), the entry
    point and tile argument of every ``tile``, and what was asked of the copy, in which order."""
    has_gi, has_w = layout == "csr", layout != "packed"
    n = 0
    for n_pairs, buildable, share, cap, codable in itertools.product(N_PAIRS, (True, False), SHARES, WINDOW_CAPS, (True, False)):
        for n_fields, compact, packed in itertools.product(range(1, 9), (False, True), (False, True)):
            old_src = Source(Copy(cap, share, codable) if buildable else None)
            new_src = Source(Copy(cap, share, codable) if buildable else None)
            what = (layout, n_pairs, buildable, share, cap, codable, n_fields, compact, packed)
            c, window, stream = parent_gridder(layout, n_pairs, old_src, n_fields, compact, packed)
            got = pp.choose_pass(n_fields, n_pairs, has_gi, has_w, compact, packed, new_src)
            assert isinstance(got, tuple) and got == pp.PassChoice(*got)            # immutable
            assert (got.use_compact, got.window, got.packed_stream) == (c is not None, window, stream), what
            assert (got.copy is new_src.copy and got.copy is not None) if got.use_compact else got.copy is None, what
            assert got.kernel == parent_apply(0, stream, c is not None, layout)[0], what
            assert new_src.asked == old_src.asked, what
            if buildable:
                assert new_src.copy.calls == old_src.copy.calls, what
            for tile in TILES:
                assert (pp.tile_override(tile, got.packed_stream, got.use_compact, has_w)
                        == parent_apply(tile, stream, c is not None, layout)), what + (tile,)
            # the products route of a group of this size through this gridder
            columns = pp.has_columns_kernel(got.use_compact, got.packed_stream, n_fields)
            for fused, profile in itertools.product((None, False, True), (False, True)):
                assert (pp.run_fused(columns, profile, n_fields, fused)
                        == parent_run_fused(c is None, stream, n_fields, profile, n_fields, fused)), what + (fused, profile)
            n += 1
    assert n == 4 * 2 * 3 * 5 * 2 * 8 * 2 * 2


def test_tile_override_on_gridders_assigned_after_construction():
    """Tools and tests assign ``compact`` / ``packed_stream`` / ``tile`` after construction: every combination of the four
    inputs, not only those ``choose_pass`` produces."""
    for tile, stream, has_compact, layout in itertools.product(TILES + (192, 256, 320, 1999, 2000), (False, True),
                                                               (False, True), LAYOUTS):
        assert pp.tile_override(tile, stream, has_compact, layout != "packed") == parent_apply(tile, stream, has_compact, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_pass_sizes_are_the_parents(layout):
    for n_pairs, buildable, cap, codable, use_compact in itertools.product(N_PAIRS, (True, False), WINDOW_CAPS, (True, False),
                                                                           (False, True)):
        what = (layout, n_pairs, buildable, cap, codable, use_compact)
        for new, old in ((pp.fields_per_pass, parent_fields_per_pass), (pp.volumes_per_pass_cap, parent_volumes_per_pass_cap)):
            old_src = Source(Copy(cap, 0.5, codable) if buildable else None)            # the fall-back share plays no part
            new_src = Source(Copy(cap, 0.5, codable) if buildable else None)
            assert new(n_pairs, layout != "packed", use_compact, new_src) == old(layout, n_pairs, old_src, use_compact), what
            assert (new_src.asked > 0) == (old_src.asked > 0), what
            if buildable:
                assert set(new_src.copy.calls) == set(old_src.copy.calls) <= {"ensure_packed"}, what
    # 8 iff the window holds 40-byte entries in 32 KiB: 819 entries
    for cap, want in ((768, 8), (819, 8), (820, 4), (1792, 4)):
        assert pp.fields_per_pass(10 ** 9, True, True, Source(Copy(cap))) == want


def test_use_compact_is_the_parents_and_asks_for_memory_last():
    edge = 160_000_000 + 8 * GIB            # 3.2 bytes per pair of 50 M pairs + 8 GiB
    for cached, n_pairs, free in itertools.product((None, False, True), N_PAIRS, (0, edge - 1, edge, edge + 1, 1 << 40)):
        asked_old, asked_new = [], []
        old = parent_use_compact(cached, n_pairs, lambda: asked_old.append(1) or free)
        new = pp.use_compact(cached, n_pairs, lambda: asked_new.append(1) or free)
        assert new is old or new == old, (cached, n_pairs, free)
        assert asked_new == asked_old == ([1] if cached is None and n_pairs >= 50_000_000 else []), (cached, n_pairs, free)
    assert [pp.use_compact(None, 50_000_000, lambda: f) for f in (edge - 1, edge, edge + 1)] == [False, False, True]


# ---- memory ------------------------------------------------------------------------------------------------------------------
def test_memory_predicates_at_their_edges():
    n = 50_000_000
    edge = 160_000_000 + 8 * GIB            # the compact copy: MORE than 3.2 B/pair + 8 GiB
    assert [pp.compact_copy_fits(n, f) for f in (edge - 1, edge, edge + 1)] == [False, False, True]
    edge = 280_000_000 + 6 * GIB            # the packed records: at least 5.6 B/pair + 6 GiB
    assert [pp.packed_records_fit(n, f) for f in (edge - 1, edge, edge + 1)] == [False, True, True]
    rec, tries, grids = 44_000_000_001, 4, 4 * 3 * 1000     # settling: three more copies, the grids, 8 GiB
    edge = 3 * rec + grids + 8 * GIB
    assert [pp.settle_copies_fit(rec, tries, grids, f) for f in (edge - 1, edge, edge + 1)] == [False, True, True]
    assert pp.compact_copy_fits(0, 8 * GIB + 1) and not pp.compact_copy_fits(0, 8 * GIB)
    assert pp.packed_records_fit(0, 6 * GIB) and not pp.packed_records_fit(0, 6 * GIB - 1)


def test_choose_layout_at_its_edges():
    n = 50_000_000
    edge = 520_000_000 + 10 * GIB           # the reference's arrays + compact copy: 10.4 B/pair + 10 GiB at most
    frees = (edge - 1, edge, edge + 1)
    assert [pp.choose_layout(n, f, False) for f in frees] == ["compact", "csr", "csr"]
    assert [pp.choose_layout(n, f, True) for f in frees] == ["packed"] * 3
    assert pp.choose_layout(n, 0, True) == "packed"
    below = 10.4 * (n - 1) + 10 * GIB       # one pair fewer: codable weights no longer matter
    assert below < edge
    for codable in (False, True):
        assert [pp.choose_layout(n - 1, f, codable) for f in frees] == ["csr"] * 3
        assert pp.choose_layout(n - 1, int(below) - 11, codable) == "compact"
        assert pp.choose_layout(0, 10 * GIB - 1, codable) == "compact" and pp.choose_layout(0, 10 * GIB, codable) == "csr"


def test_weight_code_base():
    """By hand from ``lo <= 0 or hi - base > 7 or hi >= 255`` with ``base = lo & ~7``."""
    assert pp.weight_code_base(0, 5) is None            # zero or denormal weights
    assert pp.weight_code_base(120, 127) == 120         # eight binades above a multiple of 8
    assert pp.weight_code_base(120, 128) is None        # nine
    assert pp.weight_code_base(121, 127) == 120         # Barnes
    assert pp.weight_code_base(127, 127) == 120         # uniform
    assert pp.weight_code_base(248, 255) is None        # infinities / NaN


# ---- laziness ----------------------------------------------------------------------------------------------------------------
def test_the_expensive_things_are_asked_only_when_needed():
    # a full CSR with compact=False never asks for the copy
    src = Source(Copy())
    got = pp.choose_pass(3, 10 ** 9, True, True, False, True, src)
    assert src.asked == 0 and src.copy.calls == [] and got == pp.PassChoice(pp.KERNEL_STANDARD, 0, False, False, None)
    # nor does an empty geometry, whatever it holds
    for has_gi, has_w in ((True, True), (False, True), (False, False)):
        src = Source(Copy())
        assert pp.choose_pass(1, 0, has_gi, has_w, True, True, src).kernel == pp.KERNEL_STANDARD and src.asked == 0
    # a small geometry never asks for free memory

    def no_memory():
        raise AssertionError("free memory asked")
    assert pp.use_compact(None, 49_999_999, no_memory) is False
    assert pp.use_compact(True, 10 ** 9, no_memory) is True and pp.use_compact(False, 10 ** 9, no_memory) is False
    # ensure_packed is not asked after the copy was turned down
    src = Source(Copy(share=0.0201))
    got = pp.choose_pass(1, 10 ** 9, True, True, True, True, src)
    assert not got.use_compact and src.asked == 1 and src.copy.calls == [("fallback_fraction", 768)]
    # packed=False on a full CSR never asks ensure_packed
    src = Source(Copy())
    got = pp.choose_pass(1, 10 ** 9, True, True, True, False, src)
    assert got.kernel == pp.KERNEL_TILE and src.copy.calls == [("fallback_fraction", 768)]
    # a geometry without gate_indices is not asked for its fall-back share; one without weights is always asked for records
    src = Source(Copy(window_cap=8192, share=1.0))
    got = pp.choose_pass(8, 10 ** 9, False, False, False, False, src)
    assert got == pp.PassChoice(pp.KERNEL_ROWWISE, 1216, True, True, src.copy) and src.copy.calls == ["ensure_packed"]


def test_the_thresholds_are_the_parents_literals():
    assert (pp.LARGE_GEOMETRY_PAIRS, pp.TILE_WINDOW_MAX_BYTES, pp.MAX_FALLBACK_SHARE) == (50_000_000, 24576, 0.02)
    assert pp.PIPELINE_TILES == (128, 192, 256, 320, 384, 512)
    assert (pp.COLUMNS_MIN_WORKGROUPS, pp.COLUMNS_FUSE_MIN_FIELDS, pp.COLUMNS_MAX_FIELDS) == (8192, 5, 4)
    assert (pp.LDS_BUDGET_BYTES, pp.LDS_BUDGET_ROWWISE_BYTES) == (32 << 10, 48 << 10)
    assert [pp.column_pieces(nz, cols) for nz, cols in ((20, 1), (20, 1024), (20, 8192), (20, 10 ** 6), (3, 0))] == [20, 8, 1, 1, 3]


def test_the_module_imports_without_torch_and_without_the_library():
    code = ("import sys\n"
            "import radar_processor_amd.pass_policy as pp\n"
            "from radar_processor_amd import _native\n"
            "assert 'torch' not in sys.modules, 'torch was imported'\n"
            "assert _native._lib is None, 'the library was loaded'\n"
            "assert not hasattr(pp, 'torch') and not hasattr(pp, 'load_library')\n"
            "print(pp.choose_layout(1, 0, True))\n")
    env = dict(os.environ, PYTHONPATH=REPO, HIP_VISIBLE_DEVICES="")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=REPO)
    assert res.returncode == 0 and res.stdout.strip() == "compact", res.stderr
