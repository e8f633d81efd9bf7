"""Host mirror of ``csrc/rg_compact_layout.hpp``: the layout of the compact CSR copy, written down once.

:class:`ChunkLayout` mirrors ``rgl::ChunkGrid`` -- chunks, balanced segments, the block -> segment maps of the dispatch
order and of the column mode, the segment edges of a grid's row pointers and what follows from them (pairs per chunk,
record pointers, the column mode's workgroup weights).  :func:`unpack_records` is the inverse of
``rg_csr_compact_pack_dense`` (both record codings) and :func:`check_sidecar` validates a stored layout against it.
Everything is integer arithmetic on int64 tensors of whatever device they live on; CPU tensors work.
``grid_geometry.CompactCSR`` holds the arrays and delegates here.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _native


class ChunkLayout:
    """The chunk grid of ``grid_shape`` = (planes, lines per plane, rows per line), named as ``rgl::ChunkGrid`` names it:
    ``nsx`` segments per line, the first ``seg_extra`` of ``seg_base + 1`` rows and the others of ``seg_base``; ``nyg``
    groups of ``lines`` = ``RG_COMPACT_LINES`` lines per plane; chunk ``(plane * nyg + yg) * nsx + sx``.  ``plane0``: the
    grid is a slab of whole planes of a larger one and this is its first plane there -- lines, chunks and slots stay the
    slab's own, the dispatch order's rotation counts the ``grp0 = plane0 * nyg`` line groups in front of it.  Immutable."""

    __slots__ = ("nz", "ny", "nx", "nsx", "nyg", "n_chunks", "lines", "seg_base", "seg_extra", "rot_step", "grp0")

    def __init__(self, grid_shape, plane0: int = 0):
        nz, ny, nx = (int(v) for v in grid_shape)
        lines = _native.RG_COMPACT_LINES
        nsx, nyg = (nx + 63) // 64, (ny + lines - 1) // lines
        seg_base, seg_extra = divmod(nx, max(nsx, 1))
        values = (nz, ny, nx, nsx, nyg, nz * nyg * nsx, lines, seg_base, seg_extra, _native.RG_COMPACT_ROTATION, int(plane0) * nyg)
        for name, value in zip(self.__slots__, values):
            object.__setattr__(self, name, value)

    def __setattr__(self, name, value):
        raise AttributeError("a ChunkLayout is immutable")

    def _arange(self, n: int, dev):
        torch = _native.torch_mod()
        return torch.arange(n, device=dev, dtype=torch.int64)

    # ---- segments and chunks (chunk_segment) ---------------------------------------------------------------------------
    def segment_starts(self):
        """First row of each of a line's ``nsx`` segments (+ ``nx`` as the last entry), exactly as the kernels cut them."""
        return [sx * self.seg_base + min(sx, self.seg_extra) for sx in range(self.nsx + 1)]

    def segment_rows(self, dev):
        """Rows of every segment of a line: int64 ``[nsx]``."""
        torch = _native.torch_mod()
        starts = torch.tensor(self.segment_starts(), device=dev, dtype=torch.int64)
        return starts[1:] - starts[:-1]

    def segment_of_x(self, x):
        """Segment of every position ``x`` in a line (int64 tensor)."""
        split = self.seg_extra * (self.seg_base + 1)                  # rows covered by the longer segments
        return (x // (self.seg_base + 1)).where(x < split, self.seg_extra + (x - split) // max(self.seg_base, 1))

    def line_group(self, line):
        """Line group of every line, both counted through all planes."""
        return (line // self.ny) * self.nyg + (line % self.ny) // self.lines

    def chunk_of_rows(self, rows):
        """Chunk number of every (flat, int64 tensor) row index."""
        line = rows // self.nx
        return self.line_group(line) * self.nsx + self.segment_of_x(rows - line * self.nx)

    def segment_chunks(self, dev):
        """Chunk of every (line, segment): int64 ``[lines, nsx]``."""
        return self.line_group(self._arange(self.nz * self.ny, dev))[:, None] * self.nsx + self._arange(self.nsx, dev)[None, :]

    # ---- the two block -> segment maps -----------------------------------------------------------------------------------
    def rotation(self, grp):
        """Columns both maps rotate line group ``grp`` by: ``grp * rot_step`` wraps at 32 bits, as in the kernels."""
        return ((grp * self.rot_step) & 0xFFFFFFFF) % self.nsx

    def block_chunk(self, bid):
        """Dispatch order (``block_chunk``, rg_compact_layout.hpp:117-122): the chunk workgroup ``bid`` takes -- its column
        rotated by the line group counted through all planes, plus ``grp0``."""
        grp = bid // self.nsx
        return grp * self.nsx + (bid - grp * self.nsx + self.rotation(grp + self.grp0)) % self.nsx

    def slot_of_segments(self, line, sx, rec_order: int):
        """Slot (index into ``rec_ptr``) of segment ``sx`` of grid line ``line`` (int64 tensors, lines counted through all
        planes).  ``RG_REC_ORDER_SEGMENT``: the line-major segment number.  ``RG_REC_ORDER_DISPATCH``: ``block * lines + w``
        for the wavefront ``w`` of the workgroup ``block`` that reads the segment -- the inverse of :meth:`block_chunk`."""
        if rec_order == _native.RG_REC_ORDER_SEGMENT:
            return line * self.nsx + sx
        grp = self.line_group(line)
        col = (sx - self.rotation(grp + self.grp0)) % self.nsx       # the block column whose rotated column is sx
        return (grp * self.nsx + col) * self.lines + (line % self.ny) % self.lines

    def column_segments(self, dev):
        """Column mode (rg_csr_rowwise.hpp:137): the segment column ``c`` of line group ``yg`` walks, int64 ``[nyg, nsx]`` --
        rotated by the line group WITHIN the plane, the same on every level, and without ``grp0``."""
        return (self._arange(self.nsx, dev)[None, :] + self.rotation(self._arange(self.nyg, dev))[:, None]) % self.nsx

    def n_slots(self, rec_order: int) -> int:
        """Entries of ``rec_ptr`` less one: a slot per segment, or per wavefront of every chunk (some past a plane's end)."""
        if rec_order == _native.RG_REC_ORDER_SEGMENT:
            return self.nz * self.ny * self.nsx
        return self.n_chunks * self.lines

    # ---- what the row pointers say about the segments ------------------------------------------------------------------
    def segment_edges(self, indptr):
        """Row pointers at the segment boundaries of every line: int64 ``[lines, nsx + 1]`` (one gather from ``indptr``)."""
        torch = _native.torch_mod()
        dev, n_lines = indptr.device, self.nz * self.ny
        starts = torch.tensor(self.segment_starts(), device=dev, dtype=torch.int64)
        first = self._arange(n_lines, dev) * self.nx
        return indptr[(first[:, None] + starts[None, :]).reshape(-1)].to(torch.int64).view(n_lines, self.nsx + 1)

    def segment_spans(self, indptr):
        """Pairs of every segment: int64 ``[lines, nsx]`` (lines counted through all planes)."""
        edges = self.segment_edges(indptr)
        return edges[:, 1:] - edges[:, :-1]

    def chunk_pairs(self, indptr):
        """Pairs of every chunk, int64 ``[n_chunks]``: the segments' pairs summed over the lines of a group."""
        torch = _native.torch_mod()
        seg_pairs = self.segment_spans(indptr).view(self.nz, self.ny, self.nsx)
        pad = self.nyg * self.lines - self.ny
        if pad:
            seg_pairs = torch.cat([seg_pairs, seg_pairs.new_zeros((self.nz, pad, self.nsx))], dim=1)
        return seg_pairs.view(self.nz, self.nyg, self.lines, self.nsx).sum(dim=2).reshape(-1)

    def record_pointers(self, indptr, rec_order: int, dict_ptr=None):
        """``rec_ptr`` (int64 ``[slots + 1]``) for the row pointers of the grid, in 16-byte units laid out in slot order: a
        segment of ``n = ceil(pairs / 3)`` records takes ``ceil(14 * n / 16)`` units where its chunk's dictionary
        (``dict_ptr``, int64 ``[chunks + 1]``) has at most ``RG_DENSE_MAX_DICT`` entries and ``n`` units elsewhere --
        everywhere without ``dict_ptr``, which is also the upper bound of any layout.  ``None`` when a segment would hold
        2^27 records or more."""
        torch = _native.torch_mod()
        dev, n_lines = indptr.device, self.nz * self.ny
        n_rec_seg = (self.segment_spans(indptr) + 2) // 3
        if n_rec_seg.numel() and int(n_rec_seg.max()) >= 1 << 27:
            return None
        if dict_ptr is not None and n_rec_seg.numel():
            chunk, dp = self.segment_chunks(dev), dict_ptr.to(dev)
            dense = (dp[chunk + 1] - dp[chunk]) <= _native.RG_DENSE_MAX_DICT
            n_rec_seg = torch.where(dense, (14 * n_rec_seg + 15) // 16, n_rec_seg)
        if rec_order == _native.RG_REC_ORDER_SEGMENT:
            per_slot = n_rec_seg.reshape(-1)
        else:
            line = self._arange(n_lines, dev)[:, None].expand(n_lines, self.nsx)
            sx = self._arange(self.nsx, dev)[None, :].expand(n_lines, self.nsx)
            per_slot = torch.zeros(self.n_slots(rec_order), dtype=torch.int64, device=dev)
            per_slot[self.slot_of_segments(line, sx, rec_order).reshape(-1)] = n_rec_seg.reshape(-1)
        rec_ptr = torch.zeros(per_slot.numel() + 1, dtype=torch.int64, device=dev)
        rec_ptr[1:] = torch.cumsum(per_slot, 0)
        return rec_ptr

    def column_weights(self, chunk_pairs, z_pieces: int):
        """Pairs of every workgroup of the column mode cut into ``z_pieces`` level ranges, int64
        ``[z_pieces * nyg * nsx]`` in the kernel's numbering ``(piece * nyg + yg) * nsx + column``."""
        torch = _native.torch_mod()
        cp = chunk_pairs.view(self.nz, self.nyg, self.nsx)
        sx = self.column_segments(cp.device)
        return torch.cat([torch.gather(cp[p * self.nz // z_pieces:(p + 1) * self.nz // z_pieces].sum(dim=0), 1, sx).reshape(-1)
                          for p in range(z_pieces)])


def unpack_records(layout: ChunkLayout, indptr, rec, rec_ptr, rec_order: int, w_base: int, dict_ptr, r0: int, r1: int):
    """Positions (int64) and weights (float32) of the pairs of rows ``[r0, r1)``, unpacked from the records: the inverse of
    ``rg_csr_compact_pack_dense`` in both codings (csrc/rg_compact_layout.hpp: WIDE, 16 bytes, and DENSE, 14 bytes, chosen
    per chunk by ``dict_ptr``; ``rec_ptr`` counts 16-byte units).  The weights are bit-exact: the 26-bit code is lossless."""
    torch = _native.torch_mod()
    dev = indptr.device
    ip = indptr[r0:r1 + 1].to(torch.int64)
    rows = torch.arange(r0, r1, device=dev, dtype=torch.int64)
    line = rows // layout.nx
    sx = layout.segment_of_x(rows - line * layout.nx)
    x0 = sx * layout.seg_base + sx.clamp(max=layout.seg_extra)              # chunk_segment's x0
    seg_first_pair = indptr[line * layout.nx + x0].to(torch.int64)          # pair offset where the row's segment starts
    n = int(ip[-1] - ip[0])
    row_of_pair = torch.repeat_interleave(torch.arange(r1 - r0, device=dev), ip[1:] - ip[:-1], output_size=n)
    q = torch.arange(n, device=dev, dtype=torch.int64) + ip[0] - seg_first_pair[row_of_pair]    # offset inside the segment
    unit0 = rec_ptr[layout.slot_of_segments(line, sx, rec_order)[row_of_pair]]    # first 16-byte unit of the pair's segment
    rq, j = q // 3, q % 3
    chunk = layout.line_group(line) * layout.nsx + sx
    dense = ((dict_ptr[chunk + 1] - dict_ptr[chunk]) <= _native.RG_DENSE_MAX_DICT)[row_of_pair]
    code = torch.empty(n, dtype=torch.int64, device=dev)
    pos = torch.empty(n, dtype=torch.int64, device=dev)
    wide = ~dense
    if bool(wide.any()):
        words = rec[unit0[wide] + rq[wide]].to(torch.int64) & 0xFFFFFFFF        # [m, 4] as unsigned
        jw = j[wide]
        code[wide] = torch.where(jw == 0, words[:, 0], torch.where(jw == 1, words[:, 1], words[:, 2])) & 0x3FFFFFF
        p2 = (words[:, 0] >> 26) | ((words[:, 1] >> 26) << 6) | (((words[:, 2] >> 26) & 0xF) << 12)
        pos[wide] = torch.where(jw == 0, words[:, 3] & 0xFFFF, torch.where(jw == 1, words[:, 3] >> 16, p2))
    if bool(dense.any()):
        half = rec.view(torch.int16).reshape(-1)
        rd, jd = rq[dense], j[dense]
        h = half[(unit0[dense] * 8 + 7 * rd)[:, None] + torch.arange(7, device=dev)[None, :]].to(torch.int64) & 0xFFFF
        odd = (rd & 1) == 1
        pair_w = lambda lo, hi: h[:, lo] | (h[:, hi] << 16)                  # noqa: E731  two halfwords as one word
        w2 = torch.where(odd, pair_w(0, 5), pair_w(0, 1))
        m1 = torch.where(odd, pair_w(1, 2), pair_w(2, 3))
        m2 = torch.where(odd, pair_w(3, 4), pair_w(4, 5))
        pw = h[:, 6]
        code[dense] = torch.where(jd == 0, m1, torch.where(jd == 1, m2, w2)) & 0x3FFFFFF
        p1 = (m1 >> 26) | ((pw >> 11) << 6)
        p2 = (m2 >> 26) | ((w2 >> 26) << 6)
        pos[dense] = torch.where(jd == 0, pw & 0x7FF, torch.where(jd == 1, p1, p2))
    return pos, (code + w_base).to(torch.int32).view(torch.float32)


_SIDECAR_DTYPES = dict(dict_ptr=np.int64, dict=np.int32, chunk_pairs=np.int64, chunk_counts=np.int64, rec=np.int32,
                       rec_ptr=np.int64, local_idx=np.int16)


def check_sidecar(layout: ChunkLayout, arrays, n_pairs: int) -> Optional[str]:
    """Do the arrays of a stored device layout (``grid_geometry.save_device_layout``; NumPy, by name) have the dtypes, shapes
    and end points the kernels take for granted on a grid of this layout with ``n_pairs`` pairs?  ``None``, or one line
    that starts with the name of the array at fault."""
    for name, dtype in _SIDECAR_DTYPES.items():
        if name in arrays and arrays[name].dtype != dtype:
            return f"{name} is {arrays[name].dtype}, not {np.dtype(dtype)}"
    dict_ptr, n_dict = arrays["dict_ptr"], arrays["dict"].size
    if dict_ptr.shape != (layout.n_chunks + 1,):
        return f"dict_ptr has shape {dict_ptr.shape}, not ({layout.n_chunks + 1},)"
    if dict_ptr[0] != 0 or dict_ptr[-1] != n_dict:
        return f"dict has {n_dict} entries, dict_ptr runs from {dict_ptr[0]} to {dict_ptr[-1]}"
    for name in ("chunk_pairs", "chunk_counts"):
        if arrays[name].shape != (layout.n_chunks,):
            return f"{name} has shape {arrays[name].shape}, not ({layout.n_chunks},)"
    if "rec" in arrays:
        rec, rec_ptr, rec_order = arrays["rec"], arrays["rec_ptr"], int(arrays["rec_order"][0])
        if rec_order not in (_native.RG_REC_ORDER_SEGMENT, _native.RG_REC_ORDER_DISPATCH):
            return f"rec_order is {rec_order}, neither RG_REC_ORDER_SEGMENT nor RG_REC_ORDER_DISPATCH"
        if rec_ptr.shape != (layout.n_slots(rec_order) + 1,):
            return f"rec_ptr has shape {rec_ptr.shape}, not ({layout.n_slots(rec_order) + 1},) for record order {rec_order}"
        if rec_ptr[0] != 0 or (np.diff(rec_ptr) < 0).any():
            return "rec_ptr does not start at 0 or decreases"
        if rec.shape != (rec_ptr[-1], 4):
            return f"rec has shape {rec.shape}, not ({rec_ptr[-1]}, 4) as rec_ptr ends"
    if "local_idx" in arrays and arrays["local_idx"].shape != (n_pairs,):
        return f"local_idx has shape {arrays['local_idx'].shape}, not ({n_pairs},)"
    return None
