"""The chunk prologue of the row-wise kernel (which ``rec_ptr`` / ``dict_ptr`` / row-end entries a workgroup reads, and when it
may leave early) and its pair test against wave-uniform constants, on the hand-made geometries of
``rowwise_prologue_scenes``: first and last block of the dispatch order with and without records, wavefronts without rows, a
chunk with pairs in its fourth line only, an empty plane, rows of 0-5 and 200 pairs at every residue mod 3.

Nothing there may change a byte the kernel reads or the order of an addition, so every grid is compared BIT FOR BIT with
``oracle.csr_apply_rowwise_order`` at the same lane split: no tolerance is involved.
"""
import numpy as np
import pytest

import rowwise_prologue_scenes as scenes
from oracle import radar_grid_oracle as oracle

pytestmark = pytest.mark.gpu

LIMITS = ((0.0, 1.0), (0.0, 1.0), (0.0, 1.0))
FILL = -3.0
PREFILL = 12345.0
GUARD = 64                     # guard words in front of and behind `out`
HINTS = (0, 1, 2, 8, 64)


@pytest.fixture(scope="module")
def rg():
    import radar_processor_amd as rg
    rg.load_library()
    return rg


class _Scene:
    """One variant on the device, built by the library's own builder in both record orders; oracle grids are computed once
    per (fields, lane split) and shared."""

    def __init__(self, variant):
        import torch
        from radar_processor_amd import _native
        from radar_processor_amd.grid_geometry import CompactCSR, DeviceCSR, GridGeometry
        self.torch = torch
        self.c = c = scenes.scene(variant)
        self.shape = c["shape"]
        self.n_vox = int(np.prod(self.shape))
        self.dev = dev = torch.device("cuda")
        self.csr = DeviceCSR(torch.from_numpy(c["indptr"].astype(np.int32)).to(dev), torch.from_numpy(c["gidx"]).to(dev),
                             torch.from_numpy(c["wts"]).to(dev), int(c["gidx"].max()))
        self.indptr64 = torch.from_numpy(c["indptr"]).to(dev)
        self.compacts = {}
        for order in (_native.RG_REC_ORDER_DISPATCH, _native.RG_REC_ORDER_SEGMENT):
            compact = CompactCSR.build(self.csr, self.shape)
            compact.rec_order = order
            assert compact.ensure_packed(self.csr) and compact.row_end16 is not None
            self.compacts[order] = compact
        self.geom = GridGeometry.from_device(self.shape, LIMITS, self.csr, 17000.0,
                                             compact=self.compacts[_native.RG_REC_ORDER_DISPATCH])
        self.fields = [torch.from_numpy(f).to(dev) for f in c["fields"]]
        self.masks = [None if m is None else torch.from_numpy(m.astype(np.uint8)).to(dev) for m in c["masks"]]
        self._emu, self._gridders = {}, {}

    def gridder(self, nf, order):
        from radar_processor_amd.gridding import CsrGridder
        if (nf, order) not in self._gridders:
            gr = CsrGridder(self.geom, self.c["n_gates"], nf, device=self.dev)
            gr.compact, gr.packed_stream, gr.tile = self.compacts[order], True, 0
            gr.window = gr.compact.window_for(nf, rowwise=True)
            gr.pack(self.fields[:nf], self.masks[:nf])
            self._gridders[(nf, order)] = gr
        return self._gridders[(nf, order)]

    def emu(self, nf, hint):
        if (nf, hint) not in self._emu:
            c = self.c
            self._emu[(nf, hint)] = oracle.csr_apply_rowwise_order(
                c["indptr"], c["gidx"], c["wts"], c["fields"][:nf], c["masks"][:nf], self.shape, fill_value=FILL,
                lanes_hint=hint).reshape(nf, self.n_vox)
        return self._emu[(nf, hint)]

    def guarded(self, nf):
        t = self.torch
        buf = t.full((nf * self.n_vox + 2 * GUARD,), PREFILL, dtype=t.float32, device=self.dev)
        return buf, buf[GUARD:GUARD + nf * self.n_vox].view(nf, self.n_vox)


@pytest.fixture(scope="module")
def scene(rg):
    cache = {}

    def get(variant):
        if variant not in cache:
            cache[variant] = _Scene(variant)
        return cache[variant]
    return get


def _same_bits(got, want_np):
    got_np = got.cpu().numpy()
    if not np.array_equal(np.isnan(got_np), np.isnan(want_np)):
        return False
    live = ~np.isnan(want_np)
    return np.array_equal(got_np.view(np.int32)[live], want_np.view(np.int32)[live])


def test_scenes_reach_the_kernel_as_described(rg, scene):
    """14-byte records everywhere, every populated segment on the 16-bit row ends, ``rec_ptr`` of the dispatch order equal at
    both ends of exactly the blocks whose chunk has no pair -- the first one in both variants, the last one in "empty"."""
    from radar_processor_amd import _native
    order = scenes.dispatch_chunks()
    for variant in scenes.VARIANTS:
        s = scene(variant)
        c = s.c
        compact = s.compacts[_native.RG_REC_ORDER_DISPATCH]
        sizes = (compact.dict_ptr[1:] - compact.dict_ptr[:-1]).cpu().numpy()
        assert sizes.shape == (8,) and int(sizes.max()) <= _native.RG_DENSE_MAX_DICT
        rp = compact.rec_ptr.cpu().numpy()
        assert rp.shape == (8 * scenes.LINES + 1,)
        empty = [bool(rp[b * scenes.LINES] == rp[(b + 1) * scenes.LINES]) for b in range(8)]
        assert empty == [bool(c["chunk_pairs"][order[b]] == 0) for b in range(8)]
        assert empty[0] and empty[-1] == (variant == "empty")
        assert s.compacts[_native.RG_REC_ORDER_SEGMENT].rec_ptr.numel() == len(scenes.segments()) + 1
        table = compact.row_end16.cpu().numpy().view(np.uint16)
        for (line, sx, r0, nrows, chunk) in scenes.segments():
            assert np.array_equal(table[r0:r0 + nrows].astype(np.int64), c["indptr"][r0 + 1:r0 + nrows + 1] - c["indptr"][r0])


@pytest.mark.parametrize("nf", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("variant", scenes.VARIANTS)
def test_grid_mode_is_the_documented_add_order_bit_for_bit(rg, scene, variant, nf):
    """``rg_csr_compact_apply_packed_f32`` (no table) and ``rg_csr_compact_apply_packed_f32_ex`` (the 16-bit row ends), both
    record orders, int32 and int64 row pointers, lane splits 0, 1, 2, 8 and 64: every grid equals
    ``oracle.csr_apply_rowwise_order`` at the same split bit for bit, no voxel keeps its prefill and the guard words around
    ``out`` keep theirs."""
    from radar_processor_amd import _native
    lib = _native.load_library()
    s = scene(variant)
    for order in (_native.RG_REC_ORDER_DISPATCH, _native.RG_REC_ORDER_SEGMENT):
        gr = s.gridder(nf, order)
        args32 = gr._stream_args(FILL)
        assert args32[1] == 0 and args32[4] == order
        args64 = (_native.ptr(s.indptr64), 1) + tuple(args32[2:])
        for hint in HINTS:
            want = s.emu(nf, hint)
            tile = 2000 + hint if hint else 0
            for args in (args32, args64):
                for table in (False, True):
                    buf, out = s.guarded(nf)
                    if table:
                        _native.check(lib.rg_csr_compact_apply_packed_f32_ex(
                            *args, _native.ptr(out), gr.window, tile, _native.ptr(gr.compact.row_end16), _native.stream_ptr()),
                            "rg_csr_compact_apply_packed_f32_ex")
                    else:
                        _native.check(lib.rg_csr_compact_apply_packed_f32(
                            *args, _native.ptr(out), gr.window, tile, _native.stream_ptr()), "rg_csr_compact_apply_packed_f32")
                    where = (variant, nf, order, hint, args is args64, table)
                    assert _same_bits(out, want), where
                    assert not bool((out == PREFILL).any()), where
                    assert bool((buf[:GUARD] == PREFILL).all()) and bool((buf[-GUARD:] == PREFILL).all()), where
    # the rows of the chunks without a pair hold the fill value
    rows = np.concatenate([np.arange(r0, r0 + n) for (_, _, r0, n, ch) in scenes.segments() if s.c["chunk_pairs"][ch] == 0])
    assert (s.emu(nf, 0)[:, rows] == FILL).all()


@pytest.mark.parametrize("variant", scenes.VARIANTS)
def test_column_mode_one_field(rg, scene, variant):
    """The column-mode entry point shares the prologue (it has no early exit): its grid is the oracle's bit for bit at every
    lane split in both record orders, and its column maximum / first argmax are the oracle's planes of that grid."""
    from radar_processor_amd import _native
    s = scene(variant)
    t = s.torch
    nz, ny, nx = s.shape
    for order in (_native.RG_REC_ORDER_DISPATCH, _native.RG_REC_ORDER_SEGMENT):
        gr = s.gridder(1, order)
        for hint in HINTS:
            buf, out = s.guarded(1)
            cm = t.full((1, ny, nx), PREFILL, dtype=t.float32, device=s.dev)
            ca = t.full((1, ny, nx), -9, dtype=t.int32, device=s.dev)
            gr.apply_columns(out=out, fill_value=FILL, col_max=cm, col_arg=ca, lanes_hint=hint)
            want = s.emu(1, hint)
            assert _same_bits(out, want), (variant, order, hint)
            assert bool((buf[:GUARD] == PREFILL).all()) and bool((buf[-GUARD:] == PREFILL).all())
            grid = want.reshape(nz, ny, nx)
            assert np.array_equal(cm[0].cpu().numpy(), oracle.column_max(grid, 0, nz - 1), equal_nan=True), (variant, order, hint)
            assert np.array_equal(ca[0].cpu().numpy(), oracle.column_argmax(grid, 0, nz - 1)), (variant, order, hint)
