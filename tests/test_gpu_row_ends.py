"""The row-end table of the row-wise kernel (``rg_csr_row_ends16``: two bytes per row instead of two 8-byte row pointers) and
the early exit of a workgroup whose chunk has no record, on the hand-made geometries of ``row_ends_scenes``.

The table changes where the kernel finds a row's first and last pair, never which pairs those are: every comparison of a
launch with the table against a launch without it is bit for bit.
"""
import ctypes

import numpy as np
import pytest

import row_ends_scenes as scenes
from conftest import ATOL_FRAC, RTOL
from oracle import radar_grid_oracle as oracle

pytestmark = pytest.mark.gpu

LIMITS = ((0.0, 1.0), (0.0, 1.0), (0.0, 1.0))
FILL = -3.0
PREFILL = 12345.0
GUARD = 64                     # guard words in front of and behind `out`


@pytest.fixture(scope="module")
def rg():
    import radar_processor_amd as rg
    rg.load_library()
    return rg


class _Scene:
    """One geometry on the device, built by the library's own builder in both record orders; launches and oracle results
    are computed once and shared."""

    def __init__(self, name):
        import torch
        from radar_processor_amd import _native
        from radar_processor_amd.grid_geometry import CompactCSR, DeviceCSR, GridGeometry
        self.torch, self.name = torch, name
        self.c = c = scenes.SCENES[name]()
        self.shape = c["shape"]
        self.n_vox = int(np.prod(self.shape))
        self.dev = dev = torch.device("cuda")
        self.csr = DeviceCSR(torch.from_numpy(c["indptr"].astype(np.int32)).to(dev), torch.from_numpy(c["gidx"]).to(dev),
                             torch.from_numpy(c["wts"]).to(dev), int(c["gidx"].max()))
        self.csr64 = DeviceCSR(torch.from_numpy(c["indptr"]).to(dev), self.csr.gate_indices, self.csr.weights,
                               self.csr.max_gate)
        self.compacts = {}
        for order in (_native.RG_REC_ORDER_DISPATCH, _native.RG_REC_ORDER_SEGMENT):
            compact = CompactCSR.build(self.csr, self.shape)
            compact.rec_order = order
            assert compact.ensure_packed(self.csr) and compact.row_end16 is not None
            self.compacts[order] = compact
        self.compact = self.compacts[_native.RG_REC_ORDER_DISPATCH]
        self.geom = GridGeometry.from_device(self.shape, LIMITS, self.csr, 17000.0, compact=self.compact)
        self.fields = [torch.from_numpy(f).to(dev) for f in c["fields"]]
        self.masks = [None if m is None else torch.from_numpy(m.astype(np.uint8)).to(dev) for m in c["masks"]]
        self._grid, self._emu, self._gridders = {}, {}, {}

    def gridder(self, nf, order=None, tile=0):
        from radar_processor_amd.gridding import CsrGridder
        compact = self.compact if order is None else self.compacts[order]
        key = (nf, compact.rec_order, tile)
        if key not in self._gridders:
            gr = CsrGridder(self.geom, self.c["n_gates"], nf, device=self.dev)
            gr.compact, gr.packed_stream, gr.tile = compact, True, tile
            gr.window = compact.window_for(nf, rowwise=tile != 384)
            gr.pack(self.fields[:nf], self.masks[:nf])
            self._gridders[key] = gr
        return self._gridders[key]

    def without_table(self, gr):
        """Context: the gridder's ``_ex`` entry points get a null table."""
        class _Null:
            def __enter__(self):
                self.saved, gr.compact.row_end16 = gr.compact.row_end16, None

            def __exit__(self, *exc):
                gr.compact.row_end16 = self.saved
        return _Null()

    def run(self, gr, nf, table=True, fill=FILL):
        t = self.torch
        out = t.full((nf, self.n_vox), PREFILL, dtype=t.float32, device=self.dev)
        if table:
            assert gr.compact.row_end16 is not None
            gr.apply(out, fill_value=fill)
        else:
            with self.without_table(gr):
                gr.apply(out, fill_value=fill)
        return out

    def grid(self, nf):
        """The grid of the default launch (table, dispatch order, lane split from the geometry)."""
        if nf not in self._grid:
            self._grid[nf] = self.run(self.gridder(nf), nf)
        return self._grid[nf]

    def emu(self, nf, hint=0):
        if (nf, hint) not in self._emu:
            c = self.c
            self._emu[(nf, hint)] = oracle.csr_apply_rowwise_order(
                c["indptr"], c["gidx"], c["wts"], c["fields"][:nf], c["masks"][:nf], self.shape, fill_value=FILL,
                lanes_hint=hint).reshape(nf, self.n_vox)
        return self._emu[(nf, hint)]

    def rows_of_chunk(self, chunk):
        return np.concatenate([np.arange(r0, r0 + nrows) for (_, _, r0, nrows, ch) in scenes.segments(self.shape) if ch == chunk])


@pytest.fixture(scope="module")
def scene(rg):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Scene(name)
        return cache[name]
    return get


def _bits_equal(t, a, b):
    return t.equal(a.view(t.int32), b.view(t.int32))


def _same_bits_np(got, want_np):
    got_np = got.cpu().numpy()
    if not np.array_equal(np.isnan(got_np), np.isnan(want_np)):
        return False
    live = ~np.isnan(want_np)
    return np.array_equal(got_np.view(np.int32)[live], want_np.view(np.int32)[live])


# ---- 1. the table ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_row_end_table_holds_the_rows_ends_of_every_16_bit_segment(rg, scene, name):
    """``row_end16[v] == indptr[v + 1] - indptr[r0]`` exactly in every segment ``CompactCSR.rows_fit16`` admits, from int32
    and from int64 row pointers and for a slab of whole planes; the others hold RG_ROW_END16_WIDE in their last entry.  The
    rule's edge lies between spans 65534 and 65535 (scene A holds both sides, and a
    segment with all its 70 000 pairs in one row), and each scene has segments on both paths and a chunk without a pair."""
    import torch
    from radar_processor_amd import _native
    from radar_processor_amd.grid_geometry import CompactCSR
    s = scene(name)
    c = s.c
    assert _native.RG_ROW_END16_MAX == scenes.ROW_END16_MAX == 65534 and _native.RG_ROW_END16_WIDE == 0xFFFF
    table = s.compact.row_end16.cpu().numpy().view(np.uint16)
    assert table.shape == (s.n_vox,)
    paths = set()
    for (line, sx, r0, nrows, chunk) in scenes.segments(s.shape):
        span = c["spans"][(line, sx)]
        fits = bool(CompactCSR.rows_fit16(span))
        assert fits == (span <= 65534)
        paths.add(fits)
        if fits:
            want = c["indptr"][r0 + 1:r0 + nrows + 1] - c["indptr"][r0]
            assert np.array_equal(table[r0:r0 + nrows].astype(np.int64), want), (line, sx)
        else:
            assert table[r0 + nrows - 1] == 0xFFFF, (line, sx)
    assert paths == {True, False}
    assert (c["chunk_pairs"] == 0).any() and np.array_equal(s.compact.chunk_pairs.cpu().numpy(), c["chunk_pairs"])
    if name == "A":
        for line, span in enumerate(scenes.EDGE_SPANS):
            assert c["spans"][(line, 0)] == span
        assert [bool(CompactCSR.rows_fit16(v)) for v in scenes.EDGE_SPANS] == [True, False, False, False]
        assert {0, 1, scenes.ONE_ROW_PAIRS} <= set(c["spans"].values()) and c["n_pairs"] < 500_000
        ends = set()
        for (line, sx, r0, nrows, chunk) in scenes.segments(s.shape):
            if 1 < c["spans"][(line, sx)] <= 65534:
                ends |= {int(v) % 3 for v in c["indptr"][r0 + 1:r0 + nrows + 1] - c["indptr"][r0]}
                assert c["lengths"][r0] == 0 and c["lengths"][r0 + nrows // 2] == 0 and c["lengths"][r0 + nrows - 1] == 0
        assert ends == {0, 1, 2} and set(scenes.SHORT) <= set(np.unique(c["lengths"]))
        assert len(np.unique(c["gidx"])) <= 128
    else:
        sizes = (s.compact.dict_ptr[1:] - s.compact.dict_ptr[:-1]).cpu().numpy()
        assert (sizes > _native.RG_DENSE_MAX_DICT).sum() == 1 and sizes[0] > _native.RG_DENSE_MAX_DICT
        assert c["spans"][(0, 0)] > 65535 and c["n_gates"] == 3000
    # int64 row pointers and a slab (scene B: its second plane) write the same entries
    lib = _native.load_library()
    nz, ny, nx = s.shape
    t64 = torch.full((s.n_vox,), 7, dtype=torch.int16, device=s.dev)
    _native.check(lib.rg_csr_row_ends16(_native.ptr(s.csr64.indptr), 1, s.n_vox, nx, ny, _native.ptr(t64),
                                        _native.stream_ptr()), "rg_csr_row_ends16")
    assert torch.equal(t64, s.compact.row_end16)
    if nz > 1:
        slab = torch.full((s.n_vox,), 7, dtype=torch.int16, device=s.dev)
        first = (nz - 1) * ny * nx
        _native.check(lib.rg_csr_row_ends16(_native.ptr(s.csr64.indptr) + 8 * first, 1, ny * nx, nx, ny,
                                            _native.ptr(slab) + 2 * first, _native.stream_ptr()), "rg_csr_row_ends16")
        assert torch.equal(slab[first:], s.compact.row_end16[first:]) and bool((slab[:first] == 7).all())
    stats = s.compact.row_end_stats(s.csr.indptr)
    assert 0 < stats["empty_chunks"] < 1 and 0 < stats["segments16"] < 1 and 0 < stats["voxels16"] < 1


def test_byte_count_follows_the_host_side_rule(rg, scene):
    """``CsrGridder.compact_bytes``: 2 bytes per row of a 16-bit segment, one row pointer per row + 1 of the others, nothing
    for the chunks without a pair -- restated here from the scene's spans and ``rows_fit16``."""
    from radar_processor_amd.grid_geometry import CompactCSR
    for name in ("A", "B"):
        s = scene(name)
        gr = s.gridder(1)
        want = 0
        for (line, sx, r0, nrows, chunk) in scenes.segments(s.shape):
            if s.c["chunk_pairs"][chunk] == 0:
                continue
            want += 2 * nrows if CompactCSR.rows_fit16(s.c["spans"][(line, sx)]) else 4 * (nrows + 1)
        assert s.compact.row_pointer_bytes(s.csr.indptr) == want
        with s.without_table(gr):
            s.compact._row_ptr_bytes = {}
            none = s.compact.row_pointer_bytes(s.csr.indptr)
        s.compact._row_ptr_bytes = {}
        assert none == sum(4 * (nrows + 1) for (_, _, _, nrows, ch) in scenes.segments(s.shape) if s.c["chunk_pairs"][ch])
        assert gr.compact_bytes() - gr.compact_bytes(grid_mode=False) == want - s.compact.row_pointer_bytes(s.csr.indptr, False)
        assert s.compact.nbytes() >= 2 * s.n_vox + 16 * int(s.compact.rec.shape[0])


# ---- 2. same bits with and without -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("name", ["A", "B"])
def test_same_bits_with_and_without_the_table(rg, scene, name, nf):
    """Row-wise kernel with the table == with a null table, bit for bit: lane splits 0, 1, 8 and 64, both record orders (field 0
    carries masked gates and an unmasked NaN).  The default launch == ``oracle.csr_apply_rowwise_order`` bit for bit (one and
    three fields: the three diagnostic splits too) and agrees with the tile kernel over the same records (tile = 384, which
    grids the standard kernel's bits) to the suite's bar for two float32 summation orders (conftest: 1e-5 relative + 2e-6 *
    max |field|)."""
    from radar_processor_amd import _native
    s = scene(name)
    t = s.torch
    for order in (_native.RG_REC_ORDER_DISPATCH, _native.RG_REC_ORDER_SEGMENT):
        for hint in (0, 1, 8, 64):
            gr = s.gridder(nf, order, tile=2000 + hint if hint else 0)
            with_table = s.run(gr, nf)
            assert _bits_equal(t, with_table, s.run(gr, nf, table=False)), (name, nf, order, hint)
            if hint == 0:
                assert _bits_equal(t, with_table, s.grid(nf)), (name, nf, order)
            elif nf in (1, 3) and order == _native.RG_REC_ORDER_DISPATCH:
                assert _same_bits_np(with_table, s.emu(nf, hint)), (name, nf, hint)
    assert _same_bits_np(s.grid(nf), s.emu(nf)), (name, nf)
    assert not bool((s.grid(nf) == PREFILL).any())
    if nf <= 4:
        tile = s.run(s.gridder(nf, tile=384), nf).cpu().numpy()
        row = s.grid(nf).cpu().numpy()
        assert np.array_equal(np.isnan(tile), np.isnan(row))
        for f in range(nf):
            live = ~np.isnan(row[f])
            vals = s.c["fields"][f]
            tol = RTOL * np.abs(tile[f][live]) + ATOL_FRAC * float(np.nanmax(np.abs(vals)))
            err = np.abs(row[f][live] - tile[f][live])
            print(f"scene {name} nf {nf} field {f}: worst |row-wise - tile| / bar = {float((err / tol).max()):.4f}")
            assert (err <= tol).all(), (name, nf, f)


# ---- 3. column and planes modes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [1, 4])
@pytest.mark.parametrize("name", ["A", "B"])
def test_column_and_planes_modes_with_the_table(rg, scene, name, nf):
    """With the table the column and the planes mode store the grid mode's bits, and every plane they produce is the one a
    null table gives (they keep their path through a chunk without a pair: the epilogue runs on its fill values)."""
    s = scene(name)
    t = s.torch
    nz, ny, nx = s.shape
    gr = s.gridder(nf)
    want = s.grid(nf)

    def columns():
        out = t.full((nf, s.n_vox), PREFILL, dtype=t.float32, device=s.dev)
        cm = t.full((nf, ny, nx), PREFILL, dtype=t.float32, device=s.dev)
        ca = t.full((nf, ny, nx), -9, dtype=t.int32, device=s.dev)
        keep = t.full((nf, 1, ny, nx), PREFILL, dtype=t.float32, device=s.dev)
        gr.apply_columns(out=out, fill_value=FILL, level_planes=keep, keep_lo=nz - 1, col_max=cm, col_arg=ca)
        return out, cm, ca, keep

    def planes():
        out = t.full((nf, s.n_vox), PREFILL, dtype=t.float32, device=s.dev)
        cm = t.full((nf, ny, nx), PREFILL, dtype=t.float32, device=s.dev)
        mn = t.full((nf, ny, nx), PREFILL, dtype=t.float32, device=s.dev)
        mean = t.full((nf, ny, nx), PREFILL, dtype=t.float32, device=s.dev)
        gr.apply_planes(out=out, fill_value=FILL, col_max=cm, col_min=mn, col_mean=mean)
        return out, cm, mn, mean

    for mode in (columns, planes):
        got = mode()
        with s.without_table(gr):
            null = mode()
        assert _bits_equal(t, got[0], want), (name, nf, mode.__name__)
        for a, b in zip(got, null):
            assert t.equal(a.view(t.int32), b.view(t.int32)), (name, nf, mode.__name__)
        assert not bool((got[1] == PREFILL).any())


# ---- 4. early exit -----------------------------------------------------------------------------------------------------------------
def _guarded(t, dev, nf, n_vox):
    buf = t.full((nf * n_vox + 2 * GUARD,), PREFILL, dtype=t.float32, device=dev)
    return buf, buf[GUARD:GUARD + nf * n_vox].view(nf, n_vox)


@pytest.mark.parametrize("fill", [float("nan"), -7.0])
@pytest.mark.parametrize("name", ["A", "B"])
def test_chunk_without_a_record_is_filled_and_left(rg, scene, name, fill):
    """Every row of the chunks without a pair holds ``fill`` for every field (NaN and -7), the guard words around ``out`` keep
    their value, and every other row is what the launch with a null table stores.  Scene A's last line group is partial."""
    s = scene(name)
    t = s.torch
    empty = np.nonzero(s.c["chunk_pairs"] == 0)[0]
    assert empty.size >= 1 and (name != "A" or s.shape[1] % scenes.LINES)
    rows = t.from_numpy(np.concatenate([s.rows_of_chunk(ch) for ch in empty])).to(s.dev)
    fill_bits = int(np.array([fill], dtype=np.float32).view(np.int32)[0])
    for nf in (1, 3, 8):
        gr = s.gridder(nf)
        results = []
        for table in (True, False):
            buf, out = _guarded(t, s.dev, nf, s.n_vox)
            if table:
                gr.apply(out, fill_value=fill)
            else:
                with s.without_table(gr):
                    gr.apply(out, fill_value=fill)
            assert bool((buf[:GUARD] == PREFILL).all()) and bool((buf[-GUARD:] == PREFILL).all()), (name, nf, table)
            assert bool((out[:, rows].view(t.int32) == fill_bits).all()), (name, nf, table)
            assert not bool((out == PREFILL).any())
            results.append(out)
        assert _bits_equal(t, results[0], results[1]), (name, nf)


def test_geometry_without_any_pair(rg):
    """No pair at all, grid (1, 6, 192): every chunk leaves early, with a table and without one; all of ``out`` is ``fill``,
    the guards keep their value."""
    import torch
    from radar_processor_amd import _native
    lib = _native.load_library()
    dev = torch.device("cuda")
    nz, ny, nx = scenes.SHAPE_A
    n_vox = nz * ny * nx
    n_chunks = 2 * 3
    indptr = torch.zeros(n_vox + 1, dtype=torch.int64, device=dev)
    rec_ptr = torch.zeros(n_chunks * scenes.LINES + 1, dtype=torch.int64, device=dev)
    dict_ptr = torch.zeros(n_chunks + 1, dtype=torch.int64, device=dev)
    table = torch.full((n_vox,), 7, dtype=torch.int16, device=dev)
    _native.check(lib.rg_csr_row_ends16(_native.ptr(indptr), 1, n_vox, nx, ny, _native.ptr(table), _native.stream_ptr()),
                  "rg_csr_row_ends16")
    assert bool((table == 0).all())
    for nf, stride in ((1, 1), (3, 4), (8, 8)):
        for tab in (table, None):
            for fill in (float("nan"), -7.0):
                buf, out = _guarded(torch, dev, nf, n_vox)
                _native.check(lib.rg_csr_compact_apply_packed_f32_ex(
                    _native.ptr(indptr), 1, 0, _native.ptr(rec_ptr), _native.RG_REC_ORDER_DISPATCH, 120 << 23,
                    _native.ptr(dict_ptr), 0, n_vox, 0, nx, ny, 0, nf, stride, 0, fill, _native.ptr(out), 256, 0,
                    _native.ptr(tab), _native.stream_ptr()), "rg_csr_compact_apply_packed_f32_ex")
                bits = int(np.array([fill], dtype=np.float32).view(np.int32)[0])
                assert bool((out.view(torch.int32) == bits).all()), (nf, tab is None, fill)
                assert bool((buf[:GUARD] == PREFILL).all()) and bool((buf[-GUARD:] == PREFILL).all())


# ---- 5. the entry points without _ex -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_old_entry_points_give_the_null_table_bits(rg, scene, name):
    """``rg_csr_compact_apply_packed_f32``, ``_columns_f32`` and ``_planes_f32`` with their argument lists as they were == their
    ``_ex`` variants with a null table, bit for bit (grid, column maximum, column minimum)."""
    from radar_processor_amd import _native
    s = scene(name)
    t = s.torch
    lib = _native.load_library()
    nz, ny, nx = s.shape
    for nf in (1, 4):
        gr = s.gridder(nf)
        args = gr._stream_args(FILL)
        new = lambda shape, dt=t.float32: t.full(shape, 99, dtype=dt, device=s.dev)       # noqa: E731
        # grid mode
        old, ex = new((nf, s.n_vox)), new((nf, s.n_vox))
        _native.check(lib.rg_csr_compact_apply_packed_f32(*args, _native.ptr(old), gr.window, 0, _native.stream_ptr()), "packed")
        _native.check(lib.rg_csr_compact_apply_packed_f32_ex(*args, _native.ptr(ex), gr.window, 0, 0, _native.stream_ptr()),
                      "packed_ex")
        assert _bits_equal(t, old, ex) and _bits_equal(t, old, s.grid(nf)), (name, nf)
        # column mode
        res = []
        for fn, extra in ((lib.rg_csr_compact_apply_columns_f32, ()), (lib.rg_csr_compact_apply_columns_f32_ex, (0,))):
            out, cm, ca = new((nf, s.n_vox)), new((nf, ny, nx)), new((nf, ny, nx), t.int32)
            _native.check(fn(*args, _native.ptr(out), 0, 0, 0, _native.ptr(cm), _native.ptr(ca), 0, nz - 1, gr.window, 1, 0, 0, 0,
                             0, *extra, _native.stream_ptr()), "columns")
            res.append((out, cm, ca))
        for a, b in zip(*res):
            assert t.equal(a.view(t.int32), b.view(t.int32)), (name, nf, "columns")
        assert _bits_equal(t, res[0][0], s.grid(nf))
        # planes mode
        res = []
        for fn, extra in ((lib.rg_csr_compact_apply_planes_f32, ()), (lib.rg_csr_compact_apply_planes_f32_ex, (0,))):
            out, mn = new((nf, s.n_vox)), new((nf, ny, nx))
            req = _native.PlaneRequest(out=_native.ptr(out), col_min=_native.ptr(mn), col_lo=0, col_hi=nz - 1)
            _native.check(fn(*args, ctypes.byref(req), gr.window, 1, 0, 0, 0, 0, *extra, _native.stream_ptr()), "planes")
            res.append((out, mn))
        for a, b in zip(*res):
            assert t.equal(a.view(t.int32), b.view(t.int32)), (name, nf, "planes")
        assert _bits_equal(t, res[0][0], s.grid(nf))
