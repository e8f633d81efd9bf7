"""The host side of the compact CSR layout (compact_layout.ChunkLayout and the record codec, reached through the names
grid_geometry.CompactCSR keeps) against tests/slab_scenes.py, the independent NumPy restatement of
csrc/rg_compact_layout.hpp: chunk and slot numbering in both record orders, the slabs' rotation, the record pointers of
a grid packed whole and slab by slab, the record decoder in both codings, the column mode's workgroup weights and the
sidecar check.  CPU tensors throughout: no GPU needed."""
import numpy as np
import pytest
import torch

import slab_scenes as scenes
from radar_processor_amd.grid_geometry import CompactCSR, DeviceCSR

ORDERS = (scenes.ORDER_SEGMENT, scenes.ORDER_DISPATCH)
SHAPES = ((1, 1, 1), (1, 4, 64), (3, 17, 29), (2, 6, 150), (2, 9, 700), (3, 8, 2000), scenes.SLAB_SHAPE)


def _all_segments(shape):
    """``(line, sx)`` of every segment as int64 ``[lines, nsx]`` tensors."""
    nz, ny, nx = shape
    nsx = scenes.layout(shape)[0]
    line = torch.arange(nz * ny)[:, None].expand(nz * ny, nsx)
    sx = torch.arange(nsx)[None, :].expand(nz * ny, nsx)
    return line, sx


def _slots(shape, order, plane0=0):
    line, sx = _all_segments(shape)
    return CompactCSR.slot_of_segments(line, sx, shape, order, plane0).numpy()


@pytest.mark.parametrize("shape", SHAPES)
def test_chunks_segments_and_slots_are_the_restatement_s(shape):
    nz, ny, nx = shape
    assert CompactCSR.layout(shape) == scenes.layout(shape)
    assert CompactCSR.segment_starts(nx) == scenes.segment_starts(nx)
    rows = torch.arange(nz * ny * nx)
    assert np.array_equal(CompactCSR.chunk_of_rows(rows, shape).numpy(), scenes.chunk_of_rows(shape))
    starts = scenes.segment_starts(nx)
    for (line, sx, r0, nrows, _) in scenes.segments(shape):
        assert (r0, nrows) == (line * nx + starts[sx], starts[sx + 1] - starts[sx])
    for order in ORDERS:
        table, n_slots = scenes.slot_table(shape, order)
        got = _slots(shape, order)
        assert got.shape == (nz * ny, scenes.layout(shape)[0]) and got.max() < n_slots
        assert all(int(got[line, sx]) == slot for (line, sx), slot in table.items())


def _cuts(nz):
    """Every way the slab tests cut ``nz`` planes: one slab per plane, pairs of planes, an uneven cut, the whole grid."""
    return ([(z, z + 1) for z in range(nz)], [(z, min(z + 2, nz)) for z in range(0, nz, 2)], [(0, 1), (1, nz)], [(0, nz)])


def test_a_slab_s_slots_are_the_whole_grid_s_shifted_by_its_first_slot():
    """WINDOW_SHAPE: two line groups and three segments, so the rotation of a slab depends on its first plane."""
    shape = scenes.WINDOW_SHAPE
    nz, ny, nx = shape
    assert len({scenes.rotation_of_group(p * scenes.layout(shape)[1], scenes.layout(shape)[0]) for p in range(nz)}) > 1
    for order in ORDERS:
        whole = _slots(shape, order)
        per_plane = scenes.slot_table(shape, order)[1] // nz
        for cut in _cuts(nz):
            for (iz0, iz1) in cut:
                got = _slots((iz1 - iz0, ny, nx), order, plane0=iz0)
                assert np.array_equal(got + iz0 * per_plane, whole[iz0 * ny:iz1 * ny]), (order, iz0, iz1)


def _encoded(order):
    c = scenes.make_slab_case()
    table, n_slots = scenes.slot_table(c["shape"], order)
    stream, rec_ptr = scenes.encode_records(c, c["shape"], table, n_slots)
    return c, stream, rec_ptr


@pytest.mark.parametrize("order", ORDERS)
def test_record_pointers_whole_and_slab_by_slab(order):
    c, _, want = _encoded(order)
    nz, ny, nx = c["shape"]
    n_xy = ny * nx
    indptr, dict_ptr = torch.from_numpy(c["indptr"]), torch.from_numpy(c["dict_ptr"])
    assert np.array_equal(CompactCSR.record_pointers(indptr, c["shape"], order, dict_ptr).numpy(), want)
    # without dictionaries every record takes a unit: the upper bound the builder allocates by
    bound = CompactCSR.record_pointers(indptr, c["shape"], order).numpy()
    assert bound.size == want.size and (np.diff(bound) >= np.diff(want)).all()
    per_plane = (want.size - 1) // nz
    chunks_per_plane = (dict_ptr.numel() - 1) // nz
    for parts in scenes.SLAB_PARTITIONS:
        laid, n_units = np.zeros_like(want), 0
        for (iz0, iz1) in parts:                              # as geometry_builder._build_compact_only lays them end to end
            sizes = c["sizes"][iz0 * chunks_per_plane:iz1 * chunks_per_plane]
            dp = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
            rp = CompactCSR.record_pointers(indptr[iz0 * n_xy:iz1 * n_xy + 1], (iz1 - iz0, ny, nx), order, dp, plane0=iz0).numpy()
            s0 = iz0 * per_plane
            laid[s0 + 1:s0 + rp.size] = rp[1:] + n_units
            laid[s0] = n_units
            n_units += int(rp[-1])
        assert np.array_equal(laid, want), parts


@pytest.mark.parametrize("order", ORDERS)
def test_decoder_inverts_the_encoder_in_both_codings(order):
    c, stream, rec_ptr = _encoded(order)
    assert (c["sizes"] <= scenes.DENSE_MAX).any() and (c["sizes"] > scenes.DENSE_MAX).any()
    n_vox = int(np.prod(c["shape"]))
    compact = CompactCSR(None, torch.from_numpy(c["dict_ptr"]), torch.from_numpy(c["dict"]), int(c["sizes"].max()), 4096,
                         c["shape"], torch.from_numpy(c["chunk_pairs"]), torch.from_numpy(c["sizes"]))
    compact.rec = torch.from_numpy(stream.view(np.int32).reshape(-1, 4).copy())
    compact.rec_ptr, compact.rec_order, compact.w_base = torch.from_numpy(rec_ptr), order, scenes.W_BASE
    csr = DeviceCSR(torch.from_numpy(c["indptr"]), None, None, int(c["gidx"].max()), n_pairs=c["n_pairs"])
    pos, wts = compact._record_fields(csr, 0, n_vox)
    assert np.array_equal(pos.numpy(), c["pos"])
    assert wts.dtype == torch.float32 and np.array_equal(wts.numpy().view(np.uint32), c["wts"].view(np.uint32))
    assert np.array_equal(compact.decode(csr).numpy(), c["gidx"])
    p0, p1 = int(c["indptr"][100]), int(c["indptr"][2000])
    part = compact.decode_weights(csr, 100, 2000, rows_per_slab=300).numpy()
    assert p1 > p0 and np.array_equal(part.view(np.uint32), c["wts"][p0:p1].view(np.uint32))
    assert np.array_equal(compact.decode(csr, 100, 2000, rows_per_slab=300).numpy(), c["gidx"][p0:p1])


def test_forward_block_map_is_the_restatement_s():
    """``block_chunk``: workgroup b of the dispatch order takes the chunk whose segments lie in slots ``4 b .. 4 b + 3``."""
    from radar_processor_amd.compact_layout import ChunkLayout
    for shape in SHAPES:
        lay = ChunkLayout(shape)
        nsx, _, n_chunks = scenes.layout(shape)
        table, _ = scenes.slot_table(shape, scenes.ORDER_DISPATCH)
        chunk = lay.block_chunk(torch.arange(n_chunks)).tolist()
        chunk_of = {(line, sx): ch for (line, sx, _, _, ch) in scenes.segments(shape)}
        assert all(chunk[slot // scenes.LINES] == chunk_of[key] for key, slot in table.items())
        assert [lay.n_slots(o) for o in ORDERS] == [scenes.slot_table(shape, o)[1] for o in ORDERS]
        assert (lay.nsx, lay.nyg, lay.n_chunks, lay.lines, lay.grp0) == (*scenes.layout(shape), scenes.LINES, 0)
    assert ChunkLayout(scenes.SLAB_SHAPE, plane0=3).grp0 == 3 * scenes.layout(scenes.SLAB_SHAPE)[1]
    with pytest.raises(AttributeError):
        ChunkLayout((1, 1, 1)).nx = 2


@pytest.mark.parametrize("z_pieces", [1, 2, scenes.SLAB_SHAPE[0]])
def test_column_weights_follow_the_column_mode_s_rotation(z_pieces):
    from radar_processor_amd.compact_layout import ChunkLayout
    c = scenes.make_slab_case()
    nz, ny, nx = c["shape"]
    nsx, nyg, _ = scenes.layout(c["shape"])
    want = []
    for p in range(z_pieces):
        for yg in range(nyg):                                 # the column mode rotates by the line group WITHIN the plane
            for col in range(nsx):
                sx = (col + (yg * scenes.ROTATION) % nsx) % nsx
                want.append(sum(int(c["chunk_pairs"][(z * nyg + yg) * nsx + sx])
                                for z in range(p * nz // z_pieces, (p + 1) * nz // z_pieces)))
    got = ChunkLayout(c["shape"]).column_weights(torch.from_numpy(c["chunk_pairs"]), z_pieces)
    assert got.tolist() == want and sum(want) == c["n_pairs"]


def _sidecar(order=scenes.ORDER_DISPATCH):
    c, stream, rec_ptr = _encoded(order)
    return dict(dict_ptr=c["dict_ptr"], dict=c["dict"], chunk_pairs=c["chunk_pairs"], chunk_counts=c["sizes"],
                rec=stream.view(np.int32).reshape(-1, 4), rec_ptr=rec_ptr, rec_order=np.array([order]),
                w_base=np.array([scenes.W_BASE], dtype=np.uint32), local_idx=c["pos"].astype(np.uint16).view(np.int16))


def test_sidecar_check_names_the_array_at_fault():
    from radar_processor_amd.compact_layout import ChunkLayout, check_sidecar
    c = scenes.make_slab_case()
    lay, n_pairs = ChunkLayout(c["shape"]), c["n_pairs"]
    for order in ORDERS:
        assert check_sidecar(lay, _sidecar(order), n_pairs) is None
    plain = {k: v for k, v in _sidecar().items() if not k.startswith(("rec", "w_base"))}       # positions only, no records
    assert check_sidecar(lay, plain, n_pairs) is None
    other = _sidecar(scenes.ORDER_SEGMENT)["rec_ptr"]
    assert other.size != _sidecar()["rec_ptr"].size
    defects = {"dict_ptr": lambda a: a["dict_ptr"][:-1], "dict": lambda a: a["dict"][:-1], "rec": lambda a: a["rec"][:-1],
               "rec_ptr": lambda a: other, "chunk_pairs": lambda a: a["chunk_pairs"][:-1],
               "local_idx": lambda a: a["local_idx"][:-1]}
    for name, broken in defects.items():
        arrays = _sidecar()
        arrays[name] = broken(arrays)
        reason = check_sidecar(lay, arrays, n_pairs)
        assert isinstance(reason, str) and "\n" not in reason and reason.startswith(name + " "), (name, reason)
    arrays = _sidecar()
    arrays["rec"] = arrays["rec"].astype(np.int64)
    reason = check_sidecar(lay, arrays, n_pairs)
    assert reason.startswith("rec ") and "int64" in reason
    arrays = _sidecar()
    arrays["rec_order"] = np.array([7])
    assert check_sidecar(lay, arrays, n_pairs).startswith("rec_order ")
    arrays = _sidecar()
    arrays["rec_ptr"] = arrays["rec_ptr"][::-1].copy()
    assert check_sidecar(lay, arrays, n_pairs).startswith("rec_ptr ")
