"""The two codings of the packed records (csrc/rg_compact_layout.hpp): 14 bytes per record of three pairs in a chunk whose
dictionary has at most 2048 entries, 16 bytes elsewhere -- chosen per chunk, read by the row-wise kernel (and its column /
planes modes), the tile kernel and ``CompactCSR.decode``.

Everything here runs on small HAND-MADE compact copies: the test chooses every chunk's dictionary and every pair's
position itself (the builder's positions depend on the order in which its hash set sees the gates), so that it can put
position 2047 next to weight code 0x3FFFFFF wherever it wants.  ``slab_scenes.encode_records``, plain NumPy, is the specification of
the record stream: the pack kernel has to reproduce it byte for byte.
"""
import numpy as np
import pytest

import slab_scenes as scenes
from oracle import radar_grid_oracle as oracle

pytestmark = pytest.mark.gpu

DENSE_MAX = 2048
NZ, NY, NX = 2, 8, 130                       # 3 segments of 44 / 43 / 43 rows per line, 2 line groups per plane: 12 chunks
SHAPE = (NZ, NY, NX)
LIMITS = ((0.0, 1.0), (0.0, 1.0), (0.0, 1.0))
NSX, NYG, LINES = 3, 2, 4
N_CHUNKS = NZ * NYG * NSX
W_BASE = 120 << 23                           # the weights below span exponents 120 .. 127
CODE_MAX = 0x3FFFFFF
# dictionary entries per chunk.  Chunks are numbered (plane * NYG + line group) * NSX + segment; the dispatch order rotates
# the segments by 5 per line group, so neighbours here are neighbours there too, wherever the rotation puts them.
DICTS = {
    "dense": [2048, 5, 300, 1, 2047, 1000, 64, 2048, 17, 768, 1500, 2],
    "mixed": [2048, 2049, 100, 3000, 2048, 2049, 2500, 9, 2049, 2048, 65, 4000],
}


@pytest.fixture(scope="module")
def rg():
    import radar_processor_amd as rg
    rg.load_library()
    return rg


def _segments():
    """(line, sx, first row, rows, chunk) of every segment, line-major."""
    return scenes.segments(SHAPE)


def _make(kind):
    """Row pointers, positions, dictionaries, gate indices and weights of one geometry."""
    rng = np.random.default_rng({"dense": 41, "mixed": 42}[kind])
    sizes = np.array(DICTS[kind], dtype=np.int64)
    n_vox = NZ * NY * NX
    lengths = rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 9, 11, 14], size=n_vox)
    for (line, sx, r0, nrows, chunk) in _segments():
        lengths[r0] = 400 + (line * NSX + sx) % 7               # rows of >= 400 pairs; the next rows start at offsets 0, 1, 2
        lengths[r0 + 20] = 431
    seg_first = {(line, sx): (r0, nrows) for (line, sx, r0, nrows, _) in _segments()}
    r0, nrows = seg_first[(1, 1)]
    lengths[r0:r0 + nrows] = 0                                   # a segment without pairs
    r0, nrows = seg_first[(2, 1)]
    lengths[r0:r0 + nrows] = 0
    lengths[r0 + 3] = 2                                          # one record
    r0, nrows = seg_first[(3, 1)]
    lengths[r0:r0 + nrows] = 0
    lengths[r0] = 1
    lengths[r0 + 5] = 4                                          # two records, the second one shared by two rows
    r0, nrows = seg_first[(9, 2)]
    lengths[r0:r0 + nrows] = 0
    lengths[r0 + nrows - 1] = 7                                  # three records: the last one's load reaches the padding
    indptr = np.zeros(n_vox + 1, dtype=np.int64)
    np.cumsum(lengths, out=indptr[1:])
    n_pairs = int(indptr[-1])
    chunk_of_pair = np.empty(n_pairs, dtype=np.int64)
    for (line, sx, r0, nrows, chunk) in _segments():
        chunk_of_pair[indptr[r0]:indptr[r0 + nrows]] = chunk
    pos = (rng.integers(0, 1 << 30, size=n_pairs) % sizes[chunk_of_pair]).astype(np.int64)
    wts = (np.exp(-4.0 * rng.random(n_pairs)).astype(np.float32) + np.float32(1e-5))     # Barnes range: exponents 121 .. 127
    # planted records in the first segment (chunk 0: 2048 entries, dense in both geometries), all inside its first row of
    # 400 pairs: the extremes of both fields in every pair slot, alone and together, in even and in odd records
    top = (np.array([W_BASE + CODE_MAX], dtype=np.uint32).view(np.float32)[0], DENSE_MAX - 1)      # 1.9999999, 2047
    bottom = (np.array([W_BASE], dtype=np.uint32).view(np.float32)[0], 0)                         # 2^-7, 0
    assert sizes[0] == DENSE_MAX and lengths[0] >= 400

    def plant(q, slots, hi, lo):
        for j in range(3):
            wts[3 * q + j], pos[3 * q + j] = hi if j in slots else lo
    for parity in (0, 1):
        plant(10 + parity, (0, 1, 2), top, bottom)
        plant(12 + parity, (), top, bottom)
        for j in range(3):
            plant(20 + 2 * j + parity, (j,), top, bottom)       # one slot at the top, its neighbours at the bottom
            plant(30 + 2 * j + parity, (j,), bottom, top)       # and the other way round
    dict_ptr = np.zeros(N_CHUNKS + 1, dtype=np.int64)
    np.cumsum(sizes, out=dict_ptr[1:])
    n_gates = int(dict_ptr[-1])
    dict_ = np.concatenate([dict_ptr[c] + rng.permutation(sizes[c]) for c in range(N_CHUNKS)]).astype(np.int32)
    gidx = dict_[dict_ptr[chunk_of_pair] + pos]
    chunk_pairs = np.bincount(chunk_of_pair, minlength=N_CHUNKS).astype(np.int64)
    fields = [rng.normal(10, 20, n_gates).astype(np.float32) for _ in range(8)]
    masks = [(rng.random(n_gates) < 0.2) if k % 2 == 0 else None for k in range(8)]
    fields[1][::7] = np.nan
    fields[0][2::19] = -0.0
    return dict(kind=kind, sizes=sizes, indptr=indptr, lengths=lengths, pos=pos, wts=wts, gidx=gidx, dict_ptr=dict_ptr,
                dict=dict_, n_gates=n_gates, n_pairs=n_pairs, chunk_pairs=chunk_pairs, fields=fields, masks=masks)


def _encode(case, slot_of, n_slots):
    """The record stream as bytes + rec_ptr (16-byte units): ``slab_scenes.encode_records``, the NumPy restatement of the
    layout's description.  ``slot_of[(line, sx)]``: the segment's slot."""
    return scenes.encode_records(case, SHAPE, slot_of, n_slots, W_BASE)


class _Case:
    """One geometry on the device: the hand-made compact copy, its packed records, the fields and the reference results
    every test compares against (computed once)."""

    def __init__(self, rg, kind):
        import torch
        from radar_processor_amd.grid_geometry import CompactCSR, DeviceCSR, GridGeometry
        self.torch, self.rg = torch, rg
        self.c = c = _make(kind)
        self.dev = dev = torch.device("cuda")
        self.n_vox = NZ * NY * NX
        self.csr = DeviceCSR(torch.from_numpy(c["indptr"].astype(np.int32)).to(dev), torch.from_numpy(c["gidx"]).to(dev),
                             torch.from_numpy(c["wts"]).to(dev), int(c["gidx"].max()))
        self.compact = self.make_compact()
        self.geom = GridGeometry.from_device(SHAPE, LIMITS, self.csr, 17000.0, compact=self.compact)
        assert self.compact.ensure_packed(self.csr) and self.compact.w_base == W_BASE
        self.fields = [torch.from_numpy(f).to(dev) for f in c["fields"]]
        self.masks = [None if m is None else torch.from_numpy(m.astype(np.uint8)).to(dev) for m in c["masks"]]
        self._rowwise, self._standard, self._emu = {}, {}, {}

    def make_compact(self, rec_order=None):
        from radar_processor_amd.grid_geometry import CompactCSR
        torch, c, dev = self.torch, self.c, self.dev
        local = torch.from_numpy(c["pos"].astype(np.uint16).view(np.int16)).to(dev)
        compact = CompactCSR(local, torch.from_numpy(c["dict_ptr"]).to(dev), torch.from_numpy(c["dict"]).to(dev),
                             int(c["sizes"].max()), 4096, SHAPE, torch.from_numpy(c["chunk_pairs"]).to(dev),
                             torch.from_numpy(c["sizes"]).to(dev))
        if rec_order is not None:
            compact.rec_order = rec_order
        return compact

    def gridder(self, nf, compact=None, tile=0, window=None):
        from radar_processor_amd.gridding import CsrGridder
        gr = CsrGridder(self.geom, self.c["n_gates"], nf, device=self.dev)       # compact=False: the standard kernel
        if compact is not None:
            gr.compact, gr.packed_stream, gr.tile = compact, True, tile
            gr.window = compact.window_for(nf, rowwise=tile != 384) if window is None else window
        gr.pack(self.fields[:nf], self.masks[:nf])
        return gr

    def run(self, gr, nf):
        out = self.torch.full((nf, self.n_vox), 9.0, dtype=self.torch.float32, device=self.dev)
        gr.apply(out, fill_value=-3.0)
        return out

    def rowwise(self, nf):
        if nf not in self._rowwise:
            self._rowwise[nf] = self.run(self.gridder(nf, self.compact), nf)
        return self._rowwise[nf]

    def standard(self, nf):
        if nf not in self._standard:
            self._standard[nf] = self.run(self.gridder(nf), nf)
        return self._standard[nf]

    def emu(self, nf, hint=0):
        if (nf, hint) not in self._emu:
            c = self.c
            self._emu[(nf, hint)] = oracle.csr_apply_rowwise_order(
                c["indptr"], c["gidx"], c["wts"], c["fields"][:nf], c["masks"][:nf], SHAPE, fill_value=-3.0,
                lanes_hint=hint).reshape(nf, self.n_vox)
        return self._emu[(nf, hint)]


@pytest.fixture(scope="module")
def cases(rg):
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = _Case(rg, kind)
        return cache[kind]
    return get


def _same_bits(got, want_np):
    got_np = got.cpu().numpy()
    np.testing.assert_array_equal(np.isnan(got_np), np.isnan(want_np))
    live = ~np.isnan(want_np)
    return np.array_equal(got_np.view(np.int32)[live], want_np.view(np.int32)[live])


def test_the_hand_made_geometries_hold_what_they_promise():
    """Rows of 0, 1, 2, 3, 4 and >= 400 pairs; rows whose first pair is pair 0, 1 and 2 of a record, in even and in odd
    records; segments of 0, 1, 2 and an odd number of records; dictionaries of exactly 2048 and 2049 entries; dense and
    wide chunks as neighbours in the chunk order and in the dispatch order."""
    from radar_processor_amd import _native
    assert _native.RG_DENSE_MAX_DICT == DENSE_MAX and _native.RG_COMPACT_LINES == LINES
    for kind in ("dense", "mixed"):
        c = _make(kind)
        assert c["n_gates"] <= 76800 and set(np.unique(c["lengths"])) >= {0, 1, 2, 3, 4} and c["lengths"].max() >= 400
        seen, n_recs = set(), set()
        for (line, sx, r0, nrows, chunk) in _segments():
            p0 = c["indptr"][r0]
            n_recs.add(int((c["indptr"][r0 + nrows] - p0 + 2) // 3))
            for r in range(r0, r0 + nrows):
                if c["lengths"][r]:
                    o = int(c["indptr"][r] - p0)
                    seen.add((o % 3, (o // 3) % 2))
        assert seen == {(o, par) for o in range(3) for par in range(2)}
        assert {0, 1, 2, 3} <= n_recs and any(n % 2 and n > 3 for n in n_recs)
        dense = c["sizes"] <= DENSE_MAX
        assert dense.all() == (kind == "dense")
    sizes = np.array(DICTS["mixed"])
    assert DENSE_MAX in sizes and DENSE_MAX + 1 in sizes
    dense = sizes <= DENSE_MAX
    assert (dense[:-1] != dense[1:]).sum() >= 6                      # neighbours in the chunk order
    order = []                                                      # chunk of every block of the dispatch order
    for bid in range(N_CHUNKS):
        grp, col = divmod(bid, NSX)
        order.append(grp * NSX + (col + (grp * _native.RG_COMPACT_ROTATION) % NSX) % NSX)
    d = dense[order]
    assert (d[:-1] != d[1:]).sum() >= 6                              # ... and in the dispatch order


@pytest.mark.parametrize("kind", ["dense", "mixed"])
def test_pack_kernel_writes_the_specified_bytes_in_both_orders(rg, cases, kind):
    """``rg_csr_compact_pack_dense`` == the NumPy encoder above, byte for byte (padding included), and ``rec_ptr`` counts
    16-byte units; both record orders hold the same number of units, and an all-dense geometry takes at most 14 bytes per
    record plus one unit of rounding per segment."""
    import torch
    from radar_processor_amd import _native
    from radar_processor_amd.grid_geometry import CompactCSR
    case = cases(kind)
    line = torch.arange(NZ * NY)[:, None].expand(NZ * NY, NSX)
    sx = torch.arange(NSX)[None, :].expand(NZ * NY, NSX)
    shapes = []
    for order in (_native.RG_REC_ORDER_DISPATCH, _native.RG_REC_ORDER_SEGMENT):
        compact = case.compact if order == case.compact.rec_order else case.make_compact(order)
        assert compact.ensure_packed(case.csr)
        slots = CompactCSR.slot_of_segments(line, sx, SHAPE, order)
        n_slots = NZ * NY * NSX if order == _native.RG_REC_ORDER_SEGMENT else N_CHUNKS * LINES
        stream, rec_ptr = _encode(case.c, {(l, s): int(slots[l, s]) for l in range(NZ * NY) for s in range(NSX)}, n_slots)
        assert np.array_equal(compact.rec_ptr.cpu().numpy(), rec_ptr)
        assert compact.rec.dtype == torch.int32 and compact.rec.shape == (int(rec_ptr[-1]), 4)
        got = compact.rec.cpu().numpy().view(np.uint8).reshape(-1)
        assert got.size == stream.size
        bad = np.nonzero(got != stream)[0]
        assert bad.size == 0, f"first differing byte {bad[:8]} of {got.size} (order {order})"
        shapes.append(tuple(compact.rec.shape))
    assert shapes[0] == shapes[1]
    if kind == "dense":
        n_rec = [int((case.c["indptr"][r0 + nrows] - case.c["indptr"][r0] + 2) // 3) for (_, _, r0, nrows, _) in _segments()]
        assert shapes[0][0] * 16 <= 14 * sum(n_rec) + 16 * len(n_rec)
        assert shapes[0][0] < sum(n_rec)


@pytest.mark.parametrize("kind", ["dense", "mixed"])
def test_records_decode_to_the_arrays_they_were_packed_from(rg, cases, kind):
    """``decode`` / ``decode_weights`` / ``_record_fields`` from the records alone == the original index, weight and position
    arrays, bit for bit, for the whole grid and for a row range that starts inside a segment."""
    import torch
    from radar_processor_amd.grid_geometry import DeviceCSR
    case = cases(kind)
    c = case.c
    packed_only = case.make_compact()
    packed_only.rec, packed_only.rec_ptr, packed_only.w_base = case.compact.rec, case.compact.rec_ptr, case.compact.w_base
    packed_only.local_idx = None
    csr = DeviceCSR(case.csr.indptr, None, None, case.csr.max_gate, n_pairs=c["n_pairs"])
    pos, w = packed_only._record_fields(csr, 0, case.n_vox)
    assert np.array_equal(pos.cpu().numpy(), c["pos"])
    assert np.array_equal(w.cpu().numpy().view(np.int32), c["wts"].view(np.int32))
    assert np.array_equal(packed_only.decode(csr).cpu().numpy(), c["gidx"])
    assert np.array_equal(packed_only.decode_weights(csr).cpu().numpy().view(np.int32), c["wts"].view(np.int32))
    r0, r1 = 50, 1700
    p0, p1 = int(c["indptr"][r0]), int(c["indptr"][r1])
    assert np.array_equal(packed_only.decode(csr, r0, r1).cpu().numpy(), c["gidx"][p0:p1])
    assert np.array_equal(packed_only.decode_weights(csr, r0, r1, rows_per_slab=300).cpu().numpy().view(np.int32),
                          c["wts"][p0:p1].view(np.int32))


@pytest.mark.parametrize("nf", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("kind", ["dense", "mixed"])
def test_rowwise_kernel_keeps_its_documented_order(rg, cases, kind, nf):
    """Row-wise kernel over the records == ``oracle.csr_apply_rowwise_order`` bit for bit (the coding of a record changes
    where its bytes lie, not which pairs it holds nor the order of the adds); the same bits on the per-pair path of a
    window too small for any chunk."""
    case = cases(kind)
    row = case.rowwise(nf)
    assert _same_bits(row, case.emu(nf)), (kind, nf)
    no_window = case.run(case.gridder(nf, case.compact, window=0), nf)
    assert case.torch.equal(no_window.view(case.torch.int32), row.view(case.torch.int32)), (kind, nf)


@pytest.mark.parametrize("hint", [1, 2, 8, 64])
@pytest.mark.parametrize("kind", ["dense", "mixed"])
def test_rowwise_kernel_lane_splits(rg, cases, kind, hint):
    """1, 2, 8 and 64 lanes per row (``tile = 2000 + hint``): with one lane per row the parity of a lane's records
    alternates from batch slot to batch slot, with two and more it is fixed per row and lane.  One and three fields, bit
    for bit against the oracle's restatement of the same split."""
    case = cases(kind)
    for nf in (1, 3):
        got = case.run(case.gridder(nf, case.compact, tile=2000 + hint), nf)
        assert _same_bits(got, case.emu(nf, hint)), (kind, nf, hint)


@pytest.mark.parametrize("kind", ["dense", "mixed"])
def test_tile_kernel_over_the_records_matches_the_standard_kernel(rg, cases, kind):
    """Tile kernel (tile = 384) over the same records == ``rg_csr_apply_f32`` bit for bit, 1-4 fields, with and without its
    LDS window."""
    case = cases(kind)
    t = case.torch
    for nf in (1, 2, 3, 4):
        want = case.standard(nf)
        for window in (None, 0):
            got = case.run(case.gridder(nf, case.compact, tile=384, window=window), nf)
            assert t.equal(got.view(t.int32), want.view(t.int32)), (kind, nf, window)


@pytest.mark.parametrize("kind", ["dense", "mixed"])
def test_segment_order_gives_the_same_bits(rg, cases, kind):
    """The other record order (line-major segments): other slots, the same records, the same bits from both kernels."""
    from radar_processor_amd import _native
    case = cases(kind)
    t = case.torch
    other = case.make_compact(_native.RG_REC_ORDER_SEGMENT)
    assert other.ensure_packed(case.csr) and other.rec.shape == case.compact.rec.shape
    for nf in (1, 3):
        got = case.run(case.gridder(nf, other), nf)
        assert t.equal(got.view(t.int32), case.rowwise(nf).view(t.int32)), (kind, nf)
        got = case.run(case.gridder(nf, other, tile=384), nf)
        assert t.equal(got.view(t.int32), case.standard(nf).view(t.int32)), (kind, nf)


@pytest.mark.parametrize("kind", ["dense", "mixed"])
def test_column_and_planes_modes_give_the_rowwise_bits(rg, cases, kind):
    """Column mode and planes mode (the same template walking columns of chunks), one and three fields, one and two level
    pieces: the 3-D grid they store == the row-wise kernel's, bit for bit, and their column maximum is that grid's."""
    case = cases(kind)
    t = case.torch
    for nf in (1, 3):
        want = case.rowwise(nf)
        want_np = want.cpu().numpy().reshape(nf, NZ, NY, NX)
        gr = case.gridder(nf, case.compact)
        for pieces in (1, 2):
            col = t.full((nf, case.n_vox), 9.0, dtype=t.float32, device=case.dev)
            cm = t.empty((nf, NY, NX), dtype=t.float32, device=case.dev)
            gr.apply_columns(out=col, fill_value=-3.0, col_max=cm, z_pieces=pieces)
            assert t.equal(col.view(t.int32), want.view(t.int32)), (kind, nf, pieces, "columns")
            for f in range(nf):
                assert np.array_equal(cm[f].cpu().numpy(), oracle.column_max(want_np[f], 0, NZ - 1), equal_nan=True)
            pl = t.full((nf, case.n_vox), 9.0, dtype=t.float32, device=case.dev)
            mn = t.empty((nf, NY, NX), dtype=t.float32, device=case.dev)
            gr.apply_planes(out=pl, fill_value=-3.0, col_min=mn, z_pieces=pieces)
            assert t.equal(pl.view(t.int32), want.view(t.int32)), (kind, nf, pieces, "planes")
            for f in range(nf):
                assert np.array_equal(mn[f].cpu().numpy(), np.fmin.reduce(want_np[f], axis=0), equal_nan=True)


def test_sidecar_without_the_record_format_tag_is_refused_and_rebuilt(rg, tmp_path, caplog):
    """A device-layout sidecar carries the coding of its records (``rec_format``).  A file with the tag round-trips; a file
    without it was written when every record took 16 bytes: it is refused with a warning, the layout is derived again and
    grids the same bits."""
    import torch
    from radar_processor_amd import grid_geometry
    from radar_processor_amd.gridding import CsrGridder
    rng = np.random.default_rng(3)
    n = 6000
    gx, gy = rng.uniform(-20e3, 20e3, n).astype(np.float32), rng.uniform(-20e3, 20e3, n).astype(np.float32)
    gz = rng.uniform(0.0, 9e3, n).astype(np.float32)
    val = rng.normal(10, 20, n).astype(np.float32)
    shape, limits = (3, 9, 130), ((0.0, 8e3), (-20e3, 20e3), (-20e3, 20e3))
    geom = rg.compute_grid_geometry(gx, gy, gz, shape, limits, str(tmp_path), min_radius=900.0, beam_factor=0.05)
    dev = torch.device("cuda")
    npz, side, old = str(tmp_path / "g.npz"), str(tmp_path / "g.layout.npz"), str(tmp_path / "g.old.npz")
    rg.save_geometry(geom, npz)
    assert rg.save_device_layout(geom, side)
    with np.load(side, allow_pickle=False) as data:
        arrays = {k: data[k] for k in data.files}
    assert int(arrays["rec_format"][0]) == grid_geometry.REC_FORMAT and "rec" in arrays
    np.savez(old, **{k: v for k, v in arrays.items() if k != "rec_format"})
    f_t = torch.from_numpy(val).to(dev)

    def grid(g):
        compact = g.device_compact(dev)
        assert compact is not None and compact.ensure_packed(g.device_csr(dev))
        gr = CsrGridder(g, n, 1, device=dev)
        gr.compact, gr.window, gr.packed_stream = compact, compact.window_for(1, rowwise=True), True
        gr.pack([f_t], [None])
        out = torch.empty((1, gr.n_vox), dtype=torch.float32, device=dev)
        gr.apply(out)
        return out, compact
    want, c0 = grid(geom)
    tagged = rg.load_geometry(npz)
    assert rg.load_device_layout(tagged, side) is True
    got, c1 = grid(tagged)
    assert c1 is not c0 and torch.equal(c1.rec, c0.rec) and torch.equal(c1.rec_ptr, c0.rec_ptr)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    untagged = rg.load_geometry(npz)
    with caplog.at_level("WARNING", logger="radar_grid.geometry"):
        assert rg.load_device_layout(untagged, old) is False
    assert "another coding" in caplog.text and getattr(untagged, "_compact", None) is None
    got, c2 = grid(untagged)                                         # derived again from the reference arrays
    assert c2 is not c0 and torch.equal(got.view(torch.int32), want.view(torch.int32))
