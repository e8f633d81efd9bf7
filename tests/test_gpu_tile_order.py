"""The kernels that share ``csrc/rg_row_phase.hpp`` -- ``rg_csr_apply_f32`` (K1), the tile kernel over the plain compact copy
(``rg_csr_compact_apply_f32``) and the one over the packed records (``rg_csr_compact_apply_packed_f32``, tile = 384) -- against
``oracle.csr_apply_tile_order``, the NumPy restatement of the order the header documents, BIT FOR BIT, on the hand-made
geometries of ``tile_order_scenes`` (tile seams, every lane split, gaps, segment shapes, rows without data, special values;
``test_tile_order_scenes.py`` checks restatement and scenes on the CPU).

Every comparison here is with the restatement, never with another kernel: the siblings include the same header, so a fault in
it is invisible between them.  Same NaN pattern, and the same int32 view on every voxel that is not a NaN.
"""
import numpy as np
import pytest

import tile_order_scenes as scenes

pytestmark = pytest.mark.gpu

LIMITS = ((0.0, 1.0), (0.0, 1.0), (0.0, 1.0))
FILLS = (float("nan"), -3.0, -9999.0)
PREFILL = 12345.0
GUARD = 64                     # guard words in front of and behind `out`


@pytest.fixture(scope="module")
def rg():
    import radar_processor_amd as rg
    rg.load_library()
    return rg


@pytest.fixture(scope="module")
def rest():
    return scenes.Restatements()


class _Scene:
    """One geometry on the device: row pointers in both widths, the compact copy from the library's own builder with its packed
    records in both orders, the packed fields per field count, the restatements per (field count, tile, fill)."""

    def __init__(self, name, rest):
        import torch
        from radar_processor_amd import _native
        from radar_processor_amd.grid_geometry import CompactCSR, DeviceCSR, GridGeometry
        self.torch, self.native, self.name, self.rest = torch, _native, name, rest
        self.lib = _native.load_library()
        self.c = c = rest.scene(name)
        self.shape = c["shape"]
        self.n_vox = int(np.prod(self.shape))
        self.dev = dev = torch.device("cuda")
        self.csr = DeviceCSR(torch.from_numpy(c["indptr"].astype(np.int32)).to(dev), torch.from_numpy(c["gidx"]).to(dev),
                             torch.from_numpy(c["wts"]).to(dev), int(c["gidx"].max()))
        self.indptr64 = torch.from_numpy(c["indptr"]).to(dev)
        self.geom = GridGeometry.from_device(self.shape, LIMITS, self.csr, 17000.0)
        self.fields = [torch.from_numpy(f).to(dev) for f in c["fields"]]
        self.masks = [None if m is None else torch.from_numpy(m.astype(np.uint8)).to(dev) for m in c["masks"]]
        self._gridders, self._want, self._compacts = {}, {}, {}
        self._CompactCSR = CompactCSR

    def gridder(self, nf):
        """A ``CsrGridder`` whose ``packed`` holds the first ``nf`` fields (``rg_pack_fields_f32``)."""
        from radar_processor_amd.gridding import CsrGridder
        if nf not in self._gridders:
            gr = CsrGridder(self.geom, self.c["n_gates"], nf, device=self.dev)
            assert gr.compact is None
            gr.pack(self.fields[:nf], self.masks[:nf])
            self._gridders[nf] = gr
        return self._gridders[nf]

    def compact(self, order=None):
        """The compact copy (``CompactCSR.build``); with ``order`` its packed records in that order."""
        if order not in self._compacts:
            compact = self._CompactCSR.build(self.csr, self.shape)
            assert compact is not None
            if order is not None:
                compact.rec_order = order
                assert compact.ensure_packed(self.csr), "the scenes' weights are codable"
            self._compacts[order] = compact
        return self._compacts[order]

    def want(self, nf, tile, fill):
        key = (nf, tile, repr(fill))
        if key not in self._want:
            w = self.torch.from_numpy(self.rest.get(self.name, nf, tile, fill=fill)).to(self.dev)
            self._want[key] = (w, self.torch.isnan(w))
        return self._want[key]

    def guarded(self, nf):
        t = self.torch
        buf = t.full((nf * self.n_vox + 2 * GUARD,), PREFILL, dtype=t.float32, device=self.dev)
        return buf, buf[GUARD:GUARD + nf * self.n_vox].view(nf, self.n_vox)

    def check(self, buf, out, nf, tile, fill, what):
        """Guards untouched, no prefill left, and ``out`` == the restatement: NaN pattern and bits."""
        t = self.torch
        assert bool((buf[:GUARD] == PREFILL).all()) and bool((buf[-GUARD:] == PREFILL).all()), (self.name, what, "guards")
        assert not bool((out == PREFILL).any()), (self.name, what, "prefill survives")
        want, want_nan = self.want(nf, tile, fill)
        same = (t.isnan(out) & want_nan) | (~want_nan & ~t.isnan(out) & (out.view(t.int32) == want.view(t.int32)))
        if not bool(same.all()):
            bad = (~same).nonzero().cpu().numpy()
            rows = sorted({int(r) for r in bad[:, 1]})
            labels = {k: [int(r) for r in v if int(r) in rows] for k, v in self.c["classes"].items()}
            first = [(int(f), int(r), float(out[f, r]), float(want[f, r]), int(self.c["lengths"][r])) for f, r in bad[:8]]
            raise AssertionError(f"{self.name} {what}: {len(bad)} voxels in {len(rows)} rows differ from the restatement; "
                                 f"(field, row, got, want, pairs) {first}; classes {({k: v for k, v in labels.items() if v})}")

    # ---- launches -----------------------------------------------------------------------------------------------------------
    def k1(self, nf, variant, fill, i64=False):
        n = self.native
        gr = self.gridder(nf)
        buf, out = self.guarded(nf)
        n.check(self.lib.rg_csr_apply_f32_ex(
            n.ptr(self.indptr64 if i64 else self.csr.indptr), int(i64), n.ptr(self.csr.gate_indices), n.ptr(self.csr.weights),
            self.n_vox, self.csr.n_pairs, self.shape[2], n.ptr(gr.packed), nf, gr.stride, gr.n_gates, fill, n.ptr(out),
            variant, n.stream_ptr()), "rg_csr_apply_f32_ex")
        return buf, out

    def compact_tile(self, nf, tile, window, fill, i64=False):
        n = self.native
        gr, c = self.gridder(nf), self.compact()
        nz, ny, nx = self.shape
        buf, out = self.guarded(nf)
        n.check(self.lib.rg_csr_compact_apply_f32(
            n.ptr(self.indptr64 if i64 else self.csr.indptr), int(i64), n.ptr(c.local_idx), n.ptr(self.csr.weights),
            n.ptr(c.dict_ptr), n.ptr(c.dict), self.n_vox, self.csr.n_pairs, nx, ny, n.ptr(gr.packed), nf, gr.stride, gr.n_gates,
            fill, n.ptr(out), window, tile, n.stream_ptr()), "rg_csr_compact_apply_f32")
        return buf, out

    def packed_tile(self, nf, order, fill):
        n = self.native
        gr, c = self.gridder(nf), self.compact(order)
        nz, ny, nx = self.shape
        buf, out = self.guarded(nf)
        n.check(self.lib.rg_csr_compact_apply_packed_f32_ex(
            n.ptr(self.csr.indptr), 0, n.ptr(c.rec), n.ptr(c.rec_ptr), c.rec_order, c.w_base, n.ptr(c.dict_ptr), n.ptr(c.dict),
            self.n_vox, self.csr.n_pairs, nx, ny, n.ptr(gr.packed), nf, gr.stride, gr.n_gates, fill, n.ptr(out),
            c.window_for(nf), 384, n.ptr(c.row_end16), n.stream_ptr()), "rg_csr_compact_apply_packed_f32_ex")
        return buf, out


@pytest.fixture(scope="module")
def scene(rg, rest):
    cache = {}

    def get(name):
        if name not in cache:
            cache.clear()                     # one scene's device arrays at a time
            cache[name] = _Scene(name, rest)
        return cache[name]
    return get


# ---- K1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", scenes.DATA_SCENES)
def test_k1_adds_in_the_documented_order(scene, name):
    """``rg_csr_apply_f32_ex`` over fields packed by ``rg_pack_fields_f32``: 1..8 fields, every tile the table accepts for the
    field count and variant 0, int32 and int64 row pointers, fills NaN / -3 / -9999; ``out`` sits between guard words and is
    prefilled; two launches give the same bits."""
    s = scene(name)
    t = s.torch
    for nf in range(1, 9):
        for variant in (0,) + scenes.tiles_for(nf):
            for i64 in (False, True):
                for fill in FILLS:
                    what = f"K1 nf={nf} variant={variant} i64={i64} fill={fill}"
                    buf, out = s.k1(nf, variant, fill, i64)
                    s.check(buf, out, nf, variant, fill, what)
                    again = s.k1(nf, variant, fill, i64)[1]
                    assert t.equal(out.view(t.int32), again.view(t.int32)), (name, what, "second launch")


# ---- the tile kernel over the plain compact copy ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", scenes.DATA_SCENES)
def test_compact_tile_kernel_adds_in_the_documented_order(scene, name):
    """``rg_csr_compact_apply_f32`` over ``CompactCSR.build``'s copy: 1, 2, 3, 4, 5 and 8 fields, every tile it accepts and its
    default, values from the LDS window (``window_for``) and on the per-pair path (window 0); int64 row pointers at the
    default tile."""
    s = scene(name)
    for nf in (1, 2, 3, 4, 5, 8):
        windows = (s.compact().window_for(nf), 0)
        assert windows[0] >= 256
        for tile in (0,) + scenes.tiles_for(nf):
            for window in windows:
                for fill in FILLS[:2]:
                    buf, out = s.compact_tile(nf, tile, window, fill)
                    s.check(buf, out, nf, tile, fill, f"compact nf={nf} tile={tile} window={window} fill={fill}")
        buf, out = s.compact_tile(nf, 0, windows[0], FILLS[2], i64=True)
        s.check(buf, out, nf, 0, FILLS[2], f"compact nf={nf} int64")


# ---- the tile kernel over the packed records -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", scenes.DATA_SCENES)
def test_packed_tile_kernel_adds_in_the_documented_order(scene, name):
    """``rg_csr_compact_apply_packed_f32_ex`` with tile = 384 over the records ``ensure_packed`` builds, in both record orders:
    1..4 fields, the restatement at 384 pairs per tile.  14-byte records (chunks of at most 2048 gates) in every scene but
    wide130, which has chunks with 16-byte records as well."""
    from radar_processor_amd import _native
    s = scene(name)
    for order in (_native.RG_REC_ORDER_DISPATCH, _native.RG_REC_ORDER_SEGMENT):
        dense = s.compact(order).dense_chunks()[s.compact(order).chunk_pairs > 0]
        assert bool(dense.all()) == (name != "wide130"), "14-byte records; wide130 has 16-byte ones as well"
        for nf in range(1, 5):
            for fill in FILLS:
                buf, out = s.packed_tile(nf, order, fill)
                s.check(buf, out, nf, 384, fill, f"packed nf={nf} order={order} fill={fill}")


# ---- no pair at all --------------------------------------------------------------------------------------------------------------
def test_geometry_without_a_pair(rg, rest):
    """``n_pairs == 0``: every voxel is the fill, the guards keep their value; gate indices, weights, positions, dictionaries,
    records and packed fields may be null, as the header says."""
    import torch
    from radar_processor_amd import _native
    from radar_processor_amd.grid_geometry import CompactCSR
    lib = _native.load_library()
    dev = torch.device("cuda")
    c = rest.scene("empty")
    nz, ny, nx = c["shape"]
    n_vox = nz * ny * nx
    nsx, nyg, n_chunks = CompactCSR.layout(c["shape"])
    dict_ptr = torch.zeros(n_chunks + 1, dtype=torch.int64, device=dev)
    rec_ptr = torch.zeros(n_chunks * _native.RG_COMPACT_LINES + 1, dtype=torch.int64, device=dev)
    stream = _native.stream_ptr()

    def run(nf, fill, launch):
        buf = torch.full((nf * n_vox + 2 * GUARD,), PREFILL, dtype=torch.float32, device=dev)
        out = buf[GUARD:GUARD + nf * n_vox].view(nf, n_vox)
        launch(_native.ptr(out))
        want = rest.get("empty", nf, 0, fill=fill)
        assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32)), (nf, fill)
        assert np.array_equal(want.view(np.int32), np.full((nf, n_vox), fill, dtype=np.float32).view(np.int32))
        assert bool((buf[:GUARD] == PREFILL).all()) and bool((buf[-GUARD:] == PREFILL).all())

    for i64 in (0, 1):
        indptr = torch.zeros(n_vox + 1, dtype=torch.int64 if i64 else torch.int32, device=dev)
        ip = _native.ptr(indptr)
        for fill in FILLS:
            for nf, stride in ((1, 1), (2, 2), (3, 4), (4, 4), (5, 8), (8, 8)):
                for tile in (0,) + scenes.tiles_for(nf):
                    run(nf, fill, lambda o: _native.check(lib.rg_csr_apply_f32_ex(
                        ip, i64, 0, 0, n_vox, 0, nx, 0, nf, stride, 0, fill, o, tile, stream), "rg_csr_apply_f32_ex"))
                    run(nf, fill, lambda o: _native.check(lib.rg_csr_compact_apply_f32(
                        ip, i64, 0, 0, _native.ptr(dict_ptr), 0, n_vox, 0, nx, ny, 0, nf, stride, 0, fill, o, 256, tile, stream),
                        "rg_csr_compact_apply_f32"))
                if nf <= 4:
                    for order in (_native.RG_REC_ORDER_DISPATCH, _native.RG_REC_ORDER_SEGMENT):
                        run(nf, fill, lambda o: _native.check(lib.rg_csr_compact_apply_packed_f32_ex(
                            ip, i64, 0, _native.ptr(rec_ptr), order, 120 << 23, _native.ptr(dict_ptr), 0, n_vox, 0, nx, ny, 0, nf,
                            stride, 0, fill, o, 256, 384, 0, stream), "rg_csr_compact_apply_packed_f32_ex"))
