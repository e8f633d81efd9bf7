"""CSR geometry container and its ``.npz`` persistence -- host-side mirror of
``radar_grid/geometry.py`` (``GridGeometry`` :14-91, ``save_geometry`` :94-118, ``load_geometry`` :121-150).

Same constructor arguments, attributes, helper methods, ``__repr__`` text and on-disk keys as the reference,
so geometry files are interchangeable.  What is new is where the arrays live: the CSR can be *device
resident* (built by the GPU builder, or uploaded once and cached), because at the sizes MI355X is meant for
(tens of GB of pairs, int64 row pointers) a host copy is neither needed nor wanted.  Host views
(``.indptr`` / ``.gate_indices`` / ``.weights``) are materialised lazily on first access.
"""
from __future__ import annotations

import logging
import os
from typing import Optional, Tuple

import numpy as np

from . import _native, pass_policy
from .compact_layout import ChunkLayout, check_sidecar, unpack_records

logger = logging.getLogger("radar_grid.geometry")  # same logger name as the reference (docs/LOGGING.md:128-141)

_INT32_MAX = np.iinfo(np.int32).max
_NOT_COMPACTABLE = 0x40000000     # chunk_counts marker of rg_csr_compact_count

# Order in which the packed records of a geometry are stored (include/radargrid_hip.h: RG_REC_ORDER_*).  DISPATCH = the
# order in which the apply kernels' workgroups read them, so that a launch sweeps the array as one moving front;
# SEGMENT = line-major segments (round 2's layout, kept for A/B measurements: bench.py --rec-order segment).
DEFAULT_REC_ORDER = _native.RG_REC_ORDER_DISPATCH
# Coding of the packed records a sidecar holds (save_device_layout / load_device_layout).  2: 14-byte records in the chunks
# of at most RG_DENSE_MAX_DICT gates, 16-byte records elsewhere, rec_ptr in 16-byte units.  Files without the tag hold
# 16-byte records throughout, which no kernel of this build reads: they are refused and the layout is derived again.
REC_FORMAT = 2


class DeviceCSR:
    """CSR arrays resident in HBM (torch tensors used purely as allocations)."""

    __slots__ = ("indptr", "gate_indices", "weights", "n_vox", "n_pairs", "max_gate", "is_i64")

    def __init__(self, indptr, gate_indices, weights, max_gate: int, n_pairs: Optional[int] = None):
        self.indptr = indptr
        self.gate_indices = gate_indices   # None when the geometry was built compact-only (see CompactCSR)
        self.weights = weights             # None when it was built packed-only (weights live in CompactCSR.rec)
        self.n_vox = int(indptr.shape[0]) - 1
        self.n_pairs = int(weights.shape[0]) if weights is not None else int(n_pairs)
        self.max_gate = int(max_gate)   # largest gate index referenced (-1 when there are no pairs)
        self.is_i64 = indptr.dtype == _native.torch_mod().int64

    def nbytes(self) -> int:
        return sum(int(t.numel()) * t.element_size() for t in (self.indptr, self.gate_indices, self.weights)
                   if t is not None)


def scan_counts(counts, n_rows: int):
    """Row lengths (int32 ``[n_rows + 1]``, on the device) -> row pointers int64 ``[n_rows + 1]`` (``rg_scan_counts_i64``)."""
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = counts.device
    with torch.cuda.device(dev):
        indptr = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
        ws_bytes = int(lib.rg_scan_workspace_bytes(n_rows))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _native.check(lib.rg_scan_counts_i64(_native.ptr(counts), n_rows, _native.ptr(indptr), _native.ptr(ws), ws_bytes,
                                             _native.stream_ptr()), "rg_scan_counts_i64")
    return indptr


class CompactCSR:
    """Compact device copy of a :class:`DeviceCSR` for ``rg_csr_compact_apply_f32``.  Rows are grouped in chunks that
    cover a 2-D patch of the grid -- segment ``sx`` (rows ``[64*sx, 64*sx+64)`` of a grid line) of
    ``RG_COMPACT_LINES`` consecutive lines of one plane, chunk number ``(plane*nyg + yg)*nsx + sx`` --, each chunk's
    distinct gates are listed once (``dict`` / ``dict_ptr``) and every pair stores a 16-bit position in that list
    (``local_idx``).  A chunk with more than 65536 distinct gates (the patch around the radar on a dense scan) is
    *split*: one dictionary per wavefront behind a header of ``RG_COMPACT_LINES`` offsets, recognisable by an entry count
    above 65536.  ``indptr`` and ``weights`` are shared with the standard CSR.

    This class holds the arrays, the LDS window policy and the build; the layout arithmetic and the record decoder live in
    ``compact_layout`` (``chunks`` is the grid's :class:`~.compact_layout.ChunkLayout`), and the layout methods kept here
    (``layout``, ``segment_starts``, ``chunk_of_rows``, ``slot_of_segments``, ``record_pointers``, ``segment_spans``,
    ``_record_fields``) delegate to it."""

    __slots__ = ("local_idx", "dict_ptr", "dict", "n_dict", "max_dict", "window_cap", "grid_shape", "chunk_pairs",
                 "chunk_counts", "rec", "rec_ptr", "rec_order", "w_base", "_pack_tried", "_column_orders", "row_end16",
                 "_row_ptr_bytes", "chunks")

    def __init__(self, local_idx, dict_ptr, dict_, max_dict: int, window_cap: int, grid_shape, chunk_pairs=None,
                 chunk_counts=None):
        self.local_idx = local_idx          # int16 storage of the uint16 positions [P]
        self.dict_ptr = dict_ptr            # int64 [chunks + 1]
        self.dict = dict_                   # int32 [D]
        self.n_dict = int(dict_.shape[0])
        self.max_dict = int(max_dict)
        self.window_cap = int(window_cap)   # LDS window (entries) that covers 99.9 % of the pairs (speed only)
        self.grid_shape = tuple(int(v) for v in grid_shape)   # (planes, lines per plane, rows per line)
        self.chunks = ChunkLayout(self.grid_shape)
        self.chunk_pairs = chunk_pairs      # int64 [chunks]: pairs per chunk    } kept to choose the window for a
        self.chunk_counts = chunk_counts    # int64 [chunks]: distinct gates     } given field count (window_for)
        # packed pair stream for passes of 1-8 fields (ensure_packed): records of three pairs -- 14 bytes each in the chunks
        # of at most RG_DENSE_MAX_DICT gates, 16 bytes in the others --, or None
        self.rec = None                     # int32 [n_units, 4]: 16-byte units
        self.rec_ptr = None                 # int64 [slots + 1]: first unit of the segment in slot s (see rec_order)
        self.rec_order = DEFAULT_REC_ORDER  # RG_REC_ORDER_SEGMENT (slot = segment) / RG_REC_ORDER_DISPATCH (slot_of_segments)
        self.w_base = 0                     # weight code = float32 bits - w_base
        self._pack_tried = False
        self._column_orders = {}            # z_pieces -> workgroup order of the column kernel (gridding.CsrGridder)
        # row-end table of the row-wise kernel (build_row_ends): derived data, never stored in a sidecar
        self.row_end16 = None               # int16 storage of uint16 [n_vox]: indptr[v + 1] - indptr[first row of v's segment]
        self._row_ptr_bytes = {}            # bytes per row pointer -> row_pointer_bytes

    def nbytes(self) -> int:
        return sum(int(t.numel()) * t.element_size()
                   for t in (self.local_idx, self.dict_ptr, self.dict, self.rec, self.rec_ptr, self.row_end16) if t is not None)

    @staticmethod
    def rows_fit16(span):
        """THE rule of the row-end table (csrc/rg_csr_compact_build.hip writes by it, csrc/rg_csr_rowwise.hpp reads by it): a
        segment whose ``span`` -- its pairs, ``indptr[r0 + nrows] - indptr[r0]`` -- is at most ``RG_ROW_END16_MAX`` = 65534
        keeps its row ends in 16 bits; a longer one holds ``RG_ROW_END16_WIDE`` = 0xFFFF there (which is why 65535 itself
        does not fit) and reads the row pointers.  ``span``: an int, an array or a tensor."""
        return span <= _native.RG_ROW_END16_MAX

    def build_row_ends(self, indptr) -> None:
        """Build (once) the row-end table ``rg_csr_row_ends16`` writes from the grid's row pointers: two bytes per row that
        the row-wise kernel reads instead of ``indptr[v]`` and ``indptr[v + 1]`` in every segment :meth:`rows_fit16` admits."""
        if self.row_end16 is not None:
            return
        torch = _native.torch_mod()
        lib = _native.load_library()
        nz, ny, nx = self.grid_shape
        n_vox = nz * ny * nx
        dev = indptr.device
        table = torch.empty(max(n_vox, 1), dtype=torch.int16, device=dev)[:n_vox]
        with torch.cuda.device(dev):
            _native.check(lib.rg_csr_row_ends16(_native.ptr(indptr), int(indptr.dtype == torch.int64), n_vox, nx, ny,
                                                _native.ptr(table), _native.stream_ptr()), "rg_csr_row_ends16")
        self.row_end16 = table
        self._row_ptr_bytes = {}
        st = self.row_end_stats(indptr)
        logger.info(f"Row-end table: {2 * n_vox / 1e6:.1f} MB; {100 * st['empty_chunks']:.2f} % of the chunks hold no pair, "
                    f"{100 * st['segments16']:.3f} % of the segments and {100 * st['voxels16']:.3f} % of the voxels keep "
                    "16-bit row ends")

    def row_end_stats(self, indptr) -> dict:
        """Shares the row-end table and the early exit rest on: ``empty_chunks`` (chunks without a pair), ``segments16`` and
        ``voxels16`` (segments / voxels whose row ends fit 16 bits, by :meth:`rows_fit16`)."""
        nz, ny, nx = self.grid_shape
        fit = self.rows_fit16(self.chunks.segment_spans(indptr))
        nrows = self.chunks.segment_rows(indptr.device)
        n_chunks = max(int(self.chunk_pairs.numel()), 1)
        return {"empty_chunks": float(int((self.chunk_pairs == 0).sum()) / n_chunks),
                "segments16": float(int(fit.sum()) / max(fit.numel(), 1)),
                "voxels16": float(int((fit * nrows[None, :]).sum()) / max(nz * ny * nx, 1))}

    def row_pointer_bytes(self, indptr, grid_mode: bool = True) -> int:
        """Bytes of row pointers / row ends one launch of the row-wise kernel reads: 2 per row of a segment on the 16-bit path,
        one row pointer (``nrows + 1`` of them) per segment that reads ``indptr`` -- every segment without a table --, and
        nothing for the chunks the grid mode leaves early (no pair, dispatch order)."""
        torch = _native.torch_mod()
        ip = 8 if indptr.dtype == torch.int64 else 4
        key = (ip, bool(grid_mode))
        if key not in self._row_ptr_bytes:
            spans = self.chunks.segment_spans(indptr)
            nrows = self.chunks.segment_rows(indptr.device)
            fit = self.rows_fit16(spans) if self.row_end16 is not None else torch.zeros_like(spans, dtype=torch.bool)
            live = torch.ones_like(fit)
            if grid_mode and self.rec_order == _native.RG_REC_ORDER_DISPATCH:
                live = self.chunk_pairs.to(indptr.device)[self.chunks.segment_chunks(indptr.device)] > 0
            rows16 = int(((fit & live) * nrows[None, :]).sum())
            ptrs = int(((~fit & live) * (nrows[None, :] + 1)).sum())
            self._row_ptr_bytes[key] = 2 * rows16 + ip * ptrs
        return self._row_ptr_bytes[key]

    def ensure_packed(self, csr: "DeviceCSR") -> bool:
        """Build (once) the packed pair stream ``rg_csr_compact_apply_packed_f32`` reads: positions and weights of three
        consecutive pairs of a segment in one record -- 14 bytes where the chunk's dictionary has at most
        ``RG_DENSE_MAX_DICT`` entries (11-bit positions: 4.67 bytes per pair), 16 bytes elsewhere (5.33) instead of 6 bytes
        per pair, one 16-byte load per lane.  The weight is stored as its float32 bits minus ``w_base`` in 26 bits, which is lossless exactly when all
        weights are positive and span at most 8 binades (Barnes weights: exp(-4)+1e-5 .. 1+1e-5, 7 binades; a uniform
        weight trivially); other geometries (Cressman: weights down to 0) keep the plain arrays.  Returns whether the
        stream exists.  Costs 5.4 bytes per pair of HBM on top of the copy; skipped when that does not fit."""
        if self.rec is not None or self._pack_tried:
            return self.rec is not None
        self._pack_tried = True
        torch = _native.torch_mod()
        lib = _native.load_library()
        dev = csr.indptr.device
        if csr.n_pairs == 0 or self.local_idx is None or csr.weights is None:
            return False
        free_b, _ = torch.cuda.mem_get_info(dev)
        if not pass_policy.packed_records_fit(csr.n_pairs, free_b):
            return False
        # codable?  exponent range of the weights (float32 bits >> 23; a sign bit would show up as an exponent >= 256)
        lo, hi = None, None
        step = 1 << 28
        for p0 in range(0, csr.n_pairs, step):
            e = csr.weights[p0:p0 + step].view(torch.int32) >> 23
            a, b = int(e.min()), int(e.max())
            lo, hi = (a if lo is None else min(lo, a)), (b if hi is None else max(hi, b))
        base = pass_policy.weight_code_base(lo, hi)
        if base is None:
            logger.info(f"weights span exponents {lo}..{hi}: not codable in 26 bits above a base exponent that is a multiple "
                        "of 8, the compact copy keeps the plain arrays")
            return False
        nz, ny, nx = self.grid_shape
        rec_ptr = self.chunks.record_pointers(csr.indptr, self.rec_order, self.dict_ptr)
        if rec_ptr is None:                      # the kernels address a segment's records with 32-bit byte offsets
            logger.info("a segment holds more than 2^27 records: the compact copy keeps the plain arrays")
            return False
        n_rec = int(rec_ptr[-1])
        rec = torch.empty((max(n_rec, 1), 4), dtype=torch.int32, device=dev)[:n_rec]
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        w_base = base << 23
        with torch.cuda.device(dev):
            _native.check(lib.rg_csr_compact_pack_dense(_native.ptr(csr.indptr), int(csr.is_i64), _native.ptr(self.local_idx),
                                                        _native.ptr(csr.weights), csr.n_vox, nx, ny, _native.ptr(self.dict_ptr),
                                                        _native.ptr(rec_ptr), self.rec_order, 0, w_base, _native.ptr(rec),
                                                        _native.ptr(err), _native.stream_ptr()),
                          "rg_csr_compact_pack_dense")
        if int(err.item()):
            raise _native.NativeError(f"rg_csr_compact_pack_dense reported flag {int(err.item())}")
        self.attach_records(rec, rec_ptr, self.rec_order, w_base, csr.indptr)
        return True

    def attach_records(self, rec, rec_ptr, rec_order: int, w_base: int, indptr) -> None:
        """Take ``rec`` / ``rec_ptr`` (in ``rec_order``, weights coded above ``w_base``) as the packed pair stream of the grid
        whose row pointers are ``indptr``, and build the row-end table that goes with it."""
        self.rec, self.rec_ptr, self.rec_order, self.w_base = rec, rec_ptr, int(rec_order), int(w_base)
        self._pack_tried = True
        self.build_row_ends(indptr)
        n_pairs = max(int(indptr[-1]), 1)
        logger.info(f"Packed pair stream: {rec.numel() * 4 / 1e6:.1f} MB ({rec.numel() * 4 / n_pairs:.2f} bytes per pair; "
                    f"{100 * self.dense_fraction():.2f} % of the pairs in 14-byte records)")

    def dense_chunks(self):
        """bool ``[chunks]``: the chunks whose records are 14 bytes (at most ``RG_DENSE_MAX_DICT`` dictionary entries)."""
        return (self.dict_ptr[1:] - self.dict_ptr[:-1]) <= _native.RG_DENSE_MAX_DICT

    def dense_fraction(self) -> float:
        """Share of the pairs that lie in chunks with 14-byte records."""
        if self.chunk_pairs is None or self.chunk_pairs.numel() == 0:
            return 0.0
        total = max(int(self.chunk_pairs.sum()), 1)
        return float(int(self.chunk_pairs[self.dense_chunks()].sum()) / total)

    # ---- the layout: one-line delegates to compact_layout.ChunkLayout, kept under the names callers know ---------------------
    @staticmethod
    def layout(grid_shape):
        """``(nsx, nyg, n_chunks)`` of a grid: segments per line, line groups per plane, chunks."""
        chunks = ChunkLayout(grid_shape)
        return chunks.nsx, chunks.nyg, chunks.n_chunks

    @staticmethod
    def segment_starts(nx: int):
        """``ChunkLayout.segment_starts`` of a line of ``nx`` rows."""
        return ChunkLayout((1, 1, nx)).segment_starts()

    @staticmethod
    def chunk_of_rows(rows, grid_shape):
        """``ChunkLayout.chunk_of_rows``."""
        return ChunkLayout(grid_shape).chunk_of_rows(rows)

    @staticmethod
    def slot_of_segments(line, sx, grid_shape, rec_order: int, plane0: int = 0):
        """``ChunkLayout.slot_of_segments`` (the inverse of ``block_chunk`` in csrc/rg_compact_layout.hpp)."""
        return ChunkLayout(grid_shape, plane0).slot_of_segments(line, sx, rec_order)

    @staticmethod
    def record_pointers(indptr, grid_shape, rec_order: int, dict_ptr=None, plane0: int = 0):
        """``ChunkLayout.record_pointers`` of a whole grid, or of a slab of whole planes that starts at ``plane0``."""
        return ChunkLayout(grid_shape, plane0).record_pointers(indptr, rec_order, dict_ptr)

    @staticmethod
    def segment_spans(indptr, grid_shape):
        """``ChunkLayout.segment_spans``."""
        return ChunkLayout(grid_shape).segment_spans(indptr)

    @staticmethod
    def entry_bytes(n_fields: int, rowwise: bool = False) -> int:
        """``pass_policy.entry_bytes``: bytes of one LDS window entry of the compact kernels."""
        return pass_policy.entry_bytes(n_fields, rowwise)

    def window_for(self, n_fields: int, lds_budget_bytes: Optional[int] = None, rowwise: bool = False) -> int:
        """``pass_policy.window_for`` of this geometry's 99.9 % window: the LDS window (entries) of a pass of ``n_fields``."""
        return pass_policy.window_for(self.window_cap, n_fields, rowwise, lds_budget_bytes)

    def fallback_fraction(self, window: int) -> float:
        """Share of the pairs whose chunk holds more distinct gates than ``window`` (they gather per pair)."""
        if self.chunk_pairs is None or self.chunk_pairs.numel() == 0:
            return 0.0
        total = max(int(self.chunk_pairs.sum()), 1)
        return float(int(self.chunk_pairs[self.chunk_counts > window].sum()) / total)

    @classmethod
    def build(cls, csr: "DeviceCSR", grid_shape) -> Optional["CompactCSR"]:
        """Derive the compact copy on the device (``rg_csr_compact_count`` / ``rg_csr_compact_fill``: one workgroup per
        chunk with an LDS hash set of its gates); ``None`` when a chunk references more than 65536 distinct gates
        (positions are 16 bits; the standard kernel then stays in charge)."""
        torch = _native.torch_mod()
        dev = csr.indptr.device
        nz, ny, nx = (int(v) for v in grid_shape)
        if nz * ny * nx != csr.n_vox:
            raise ValueError(f"grid_shape {grid_shape} does not match the CSR's {csr.n_vox} rows")
        local = torch.empty(max(csr.n_pairs, 1), dtype=torch.int16, device=dev)[:csr.n_pairs]
        with torch.cuda.device(dev):
            built = cls._planes(csr.indptr, _native.ptr(csr.gate_indices), nz, ny, nx, _native.ptr(local))
        if built is None:
            return None
        counts, dict_ = built
        return cls._finish(csr.indptr, grid_shape, local, counts, [dict_])

    @staticmethod
    def _planes(indptr, gate_idx_ptr: int, n_planes: int, ny: int, nx: int, local_ptr: int):
        """Dictionaries and positions of the chunks of ``n_planes`` whole planes whose (absolute) row pointers are
        ``indptr`` (a tensor of ``n_planes*ny*nx + 1`` entries, possibly a view into a longer one).  ``gate_idx_ptr`` /
        ``local_ptr`` are device addresses such that element ``p`` belongs to absolute pair ``p``.  Returns
        ``(counts int64 [chunks], dict int32)`` with the dictionaries back to back, or ``None`` when a chunk is too
        rich."""
        torch = _native.torch_mod()
        lib = _native.load_library()
        dev = indptr.device
        n_rows = n_planes * ny * nx
        n_chunks = int(lib.rg_csr_compact_chunks(n_rows, nx, ny)) if n_rows else 0
        if n_chunks < 0:
            raise _native.NativeError("rg_csr_compact_chunks rejected the grid shape")
        if n_chunks == 0:
            return torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
        is_i64 = int(indptr.dtype == torch.int64)
        stream = _native.stream_ptr()
        counts = torch.zeros(n_chunks + 1, dtype=torch.int32, device=dev)
        rounds = torch.empty(n_chunks, dtype=torch.uint8, device=dev)
        _native.check(lib.rg_csr_compact_count(_native.ptr(indptr), is_i64, gate_idx_ptr, n_rows, nx, ny,
                                               _native.ptr(counts), _native.ptr(rounds), stream), "rg_csr_compact_count")
        if int(counts.max()) >= _NOT_COMPACTABLE:      # a single 64-row segment references more than 65536 gates
            return None
        dict_ptr = scan_counts(counts, n_chunks)
        n_dict = int(dict_ptr[-1])
        dict_ = torch.empty(max(n_dict, 1), dtype=torch.int32, device=dev)[:n_dict]
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        _native.check(lib.rg_csr_compact_fill(_native.ptr(indptr), is_i64, gate_idx_ptr, n_rows, nx, ny,
                                              _native.ptr(dict_ptr), _native.ptr(rounds), _native.ptr(dict_), local_ptr,
                                              _native.ptr(err), stream), "rg_csr_compact_fill")
        flag = int(err.item())
        if flag:
            raise _native.NativeError(f"rg_csr_compact_fill: the fill pass saw different inputs than the count pass "
                                      f"(flag {flag}); were the gate indices modified during the build?")
        return counts[:n_chunks].to(torch.int64), dict_

    @classmethod
    def _finish(cls, indptr, grid_shape, local, counts, parts) -> "CompactCSR":
        torch = _native.torch_mod()
        dev = counts.device
        chunks = ChunkLayout(grid_shape)
        n_chunks = chunks.n_chunks
        assert n_chunks == int(counts.shape[0])
        dict_ptr = torch.zeros(n_chunks + 1, dtype=torch.int64, device=dev)
        dict_ptr[1:] = torch.cumsum(counts, 0)
        dict_ = torch.cat(parts) if parts else torch.zeros(1, dtype=torch.int32, device=dev)[:0]
        chunk_pairs = chunks.chunk_pairs(indptr)             # from the row pointers at the segment edges
        # LDS window: the smallest size (multiple of 256 entries) that leaves at most 0.1 % of the pairs to the
        # per-pair fallback
        window_cap = _native.RG_COMPACT_MAX_WINDOW
        total = max(int(chunk_pairs.sum()), 1)
        for cap in range(256, _native.RG_COMPACT_MAX_WINDOW + 1, 256):
            if int(chunk_pairs[counts > cap].sum()) <= total // 1000:
                window_cap = cap
                break
        return cls(local, dict_ptr, dict_, int(counts.max()) if n_chunks else 0, window_cap, grid_shape,
                   chunk_pairs, counts)

    def _record_fields(self, csr: "DeviceCSR", r0: int, r1: int):
        """Positions (int64) and weights (float32) of the pairs of rows ``[r0, r1)``: ``compact_layout.unpack_records`` (used
        when the plain ``local_idx`` / ``weights`` arrays do not exist)."""
        return unpack_records(self.chunks, csr.indptr, self.rec, self.rec_ptr, self.rec_order, self.w_base, self.dict_ptr, r0, r1)

    def decode_weights(self, csr: "DeviceCSR", row0: int = 0, row1: Optional[int] = None, rows_per_slab: int = 500_000):
        """float32 weights of rows ``[row0, row1)``: a view of ``csr.weights`` when it exists, else unpacked from the
        records (bit-exact: the 26-bit code is lossless)."""
        torch = _native.torch_mod()
        row1 = csr.n_vox if row1 is None else row1
        q0, q1 = int(csr.indptr[row0]), int(csr.indptr[row1])
        if csr.weights is not None:
            return csr.weights[q0:q1]
        out = torch.empty(max(q1 - q0, 1), dtype=torch.float32, device=csr.indptr.device)[:q1 - q0]
        for r0 in range(row0, row1, rows_per_slab):
            r1 = min(row1, r0 + rows_per_slab)
            p0, p1 = int(csr.indptr[r0]), int(csr.indptr[r1])
            if p1 > p0:
                out[p0 - q0:p1 - q0] = self._record_fields(csr, r0, r1)[1]
        return out

    def decode(self, csr: "DeviceCSR", row0: int = 0, row1: Optional[int] = None, rows_per_slab: int = 500_000):
        """The standard int32 gate indices of rows ``[row0, row1)`` (default: all), rebuilt from positions and
        dictionaries; device tensor of ``indptr[row1] - indptr[row0]`` entries."""
        torch = _native.torch_mod()
        dev = csr.indptr.device
        row1 = csr.n_vox if row1 is None else row1
        q0, q1 = int(csr.indptr[row0]), int(csr.indptr[row1])
        out = torch.empty(max(q1 - q0, 1), dtype=torch.int32, device=dev)[:q1 - q0]
        for r0 in range(row0, row1, rows_per_slab):
            r1 = min(row1, r0 + rows_per_slab)
            ip = csr.indptr[r0:r1 + 1].to(torch.int64)
            p0, p1 = int(ip[0]), int(ip[-1])
            if p1 == p0:
                continue
            rows = torch.arange(r0, r1, device=dev, dtype=torch.int64)
            chunk_of_row = self.chunks.chunk_of_rows(rows)
            start_of_row = self.dict_ptr[chunk_of_row]
            # split chunks (more than 65536 entries: one dictionary per wavefront behind a header of offsets)
            is_split = (self.dict_ptr[chunk_of_row + 1] - start_of_row) > 65536
            if bool(is_split.any()):
                wave = ((rows // self.grid_shape[2]) % self.grid_shape[1]) % _native.RG_COMPACT_LINES
                header = self.dict[(start_of_row + wave).clamp(max=self.n_dict - 1)].to(torch.int64)
                start_of_row = start_of_row + torch.where(is_split, header, torch.zeros_like(header))
            start_of_pair = torch.repeat_interleave(start_of_row, ip[1:] - ip[:-1], output_size=p1 - p0)
            if self.local_idx is not None:
                pos = self.local_idx[p0:p1].to(torch.int64) & 0xFFFF
            else:
                pos = self._record_fields(csr, r0, r1)[0]
            out[p0 - q0:p1 - q0] = self.dict[start_of_pair + pos]
        return out


class GridGeometry:
    """Precomputed gate -> voxel mapping in CSR form (``radar_grid/geometry.py:14-52``).

    Row ``v = (iz*ny + iy)*nx + ix`` owns ``gate_indices[indptr[v]:indptr[v+1]]`` and the matching
    ``weights``.  ``indptr`` is int32 like the reference's whenever the pair count fits, int64 otherwise
    (the reference overflows there).
    """

    def __init__(self, grid_shape: Tuple[int, int, int], grid_limits, indptr, gate_indices, weights,
                 toa: float, radar_altitude: float = 0.0):
        self.grid_shape = grid_shape
        self.grid_limits = grid_limits
        self.toa = toa
        self.radar_altitude = radar_altitude
        self._indptr = indptr
        self._gate_indices = gate_indices
        self._weights = weights
        self._dev: Optional[DeviceCSR] = None

    # ---- construction from device-resident arrays (GPU builder) -----------------------------------
    @classmethod
    def from_device(cls, grid_shape, grid_limits, csr: DeviceCSR, toa: float, radar_altitude: float = 0.0,
                    compact: Optional["CompactCSR"] = None):
        g = cls(grid_shape, grid_limits, None, None, None, toa, radar_altitude)
        g._dev = csr
        if compact is not None:
            g._compact = (csr, compact)
        elif csr.gate_indices is None:
            raise ValueError("a CSR without gate indices needs its compact copy")
        return g

    # ---- host views (lazy) -----------------------------------------------------------------------
    def _host(self, name: str):
        arr = getattr(self, "_" + name)
        if arr is None:
            if self._dev is None:
                raise AttributeError(f"GridGeometry has no {name}")
            logger.debug("copying %s to the host", name)
            dev_arr = getattr(self._dev, name)
            if dev_arr is None:      # compact-only / packed-only geometry: rebuild the reference's array from the copy
                dev_arr = (self._compact[1].decode(self._dev) if name == "gate_indices"
                           else self._compact[1].decode_weights(self._dev))
            arr = dev_arr.cpu().numpy()
            setattr(self, "_" + name, arr)
        return arr

    def _assign(self, name: str, value) -> None:
        """Plain attribute assignment, as on the reference dataclass: the other two arrays are pulled to the host
        first (a device-built geometry holds its only copy in HBM), then every device-side cache -- the resident
        CSR and its compact copy -- is dropped, so the next gridding call uploads and validates the new arrays."""
        if self._dev is not None:
            for other in ("indptr", "gate_indices", "weights"):
                if other != name:
                    self._host(other)
        setattr(self, "_" + name, value)
        self.invalidate_device()

    def invalidate_device(self) -> None:
        """Forget the device-resident copies (CSR, compact copy, cached gridders).  Call this after modifying the host
        arrays IN PLACE: ``device_csr`` otherwise keeps serving the arrays it uploaded the first time."""
        if self._dev is not None:
            for name in ("indptr", "gate_indices", "weights"):
                self._host(name)
        self._dev = None
        self.__dict__.pop("_compact", None)
        self.__dict__.pop("_gridders", None)

    @property
    def indptr(self) -> np.ndarray:
        return self._host("indptr")

    @indptr.setter
    def indptr(self, value):
        self._assign("indptr", value)

    @property
    def gate_indices(self) -> np.ndarray:
        return self._host("gate_indices")

    @gate_indices.setter
    def gate_indices(self, value):
        self._assign("gate_indices", value)

    @property
    def weights(self) -> np.ndarray:
        return self._host("weights")

    @weights.setter
    def weights(self, value):
        self._assign("weights", value)

    @property
    def is_device_resident(self) -> bool:
        return self._dev is not None

    # ---- reference helper methods (geometry.py:54-91) --------------------------------------------
    def memory_usage_mb(self) -> float:
        if self._indptr is None and self._dev is not None:
            cached = getattr(self, "_compact", None)      # a compact-only / packed-only geometry lives in its copy
            extra = cached[1].nbytes() if (cached is not None and cached[1] is not None
                                           and (self._dev.gate_indices is None or self._dev.weights is None)) else 0
            return (self._dev.nbytes() + extra) / 1e6
        return (self.indptr.nbytes + self.gate_indices.nbytes + self.weights.nbytes) / 1e6

    def n_grid_points(self) -> int:
        return int(np.prod(self.grid_shape))

    def n_pairs(self) -> int:
        if self._gate_indices is None and self._dev is not None:
            return self._dev.n_pairs
        return len(self.gate_indices)

    def avg_neighbors(self) -> float:
        return self.n_pairs() / self.n_grid_points()

    def z_levels(self) -> np.ndarray:
        nz = self.grid_shape[0]
        z_min, z_max = self.grid_limits[0]
        return np.linspace(z_min, z_max, nz)

    def z_levels_absolute(self) -> np.ndarray:
        return self.z_levels() + self.radar_altitude

    def __repr__(self) -> str:
        return (
            "GridGeometry(\n"
            f"  grid_shape={self.grid_shape},\n"
            f"  grid_limits={self.grid_limits},\n"
            f"  toa={self.toa}m,\n"
            f"  radar_altitude={self.radar_altitude}m,\n"
            f"  n_pairs={self.n_pairs():,},\n"
            f"  avg_neighbors={self.avg_neighbors():.1f},\n"
            f"  memory={self.memory_usage_mb():.1f} MB\n"
            ")"
        )

    def __eq__(self, other):  # the reference is a dataclass: field-wise equality
        if not isinstance(other, GridGeometry):
            return NotImplemented
        return (tuple(self.grid_shape) == tuple(other.grid_shape) and self.grid_limits == other.grid_limits
                and self.toa == other.toa and self.radar_altitude == other.radar_altitude
                and np.array_equal(self.indptr, other.indptr)
                and np.array_equal(self.gate_indices, other.gate_indices)
                and np.array_equal(self.weights, other.weights))

    __hash__ = None

    # ---- device residency -----------------------------------------------------------------------
    def device_compact(self, device=None) -> Optional[CompactCSR]:
        """Compact copy of the device CSR (built once, cached); ``None`` when the geometry cannot be compacted."""
        csr = self.device_csr(device)
        cached = getattr(self, "_compact", None)
        if cached is not None and cached[0] is csr:
            return cached[1]
        compact = CompactCSR.build(csr, self.grid_shape)
        self._compact = (csr, compact)
        if compact is not None:
            logger.info(f"Compact CSR copy: {compact.nbytes() / 1e6:.1f} MB, {compact.n_dict:,} dictionary entries, "
                        f"largest chunk {compact.max_dict}")
        return compact

    def device_csr(self, device=None) -> DeviceCSR:
        """CSR in HBM: uploaded (and validated) once, then cached on the object."""
        dev = _native.canonical_device(device)
        if self._dev is not None and self._dev.indptr.device == dev:
            return self._dev
        torch = _native.torch_mod()
        if self._dev is not None:   # resident on another GPU: replicate device-to-device
            src = self._dev
            if src.gate_indices is None or src.weights is None:
                raise _native.NativeError("a compact-only geometry cannot be replicated to another GPU; rebuild it there")
            self._dev = DeviceCSR(src.indptr.to(dev), src.gate_indices.to(dev), src.weights.to(dev), src.max_gate)
            return self._dev
        indptr = np.ascontiguousarray(self._indptr)
        gidx = np.ascontiguousarray(self._gate_indices)
        wts = np.ascontiguousarray(self._weights)
        n_vox = self.n_grid_points()
        if indptr.ndim != 1 or indptr.shape[0] != n_vox + 1:
            raise ValueError(f"indptr has {indptr.shape[0]} entries, expected {n_vox + 1} for grid {self.grid_shape}")
        if not np.issubdtype(indptr.dtype, np.integer):
            raise ValueError("indptr must be an integer array")
        if gidx.shape[0] != wts.shape[0]:
            raise ValueError("gate_indices and weights differ in length")
        if indptr.shape[0] and (indptr[0] != 0 or indptr[-1] != gidx.shape[0] or np.any(np.diff(indptr) < 0)):
            raise ValueError("indptr must start at 0, end at len(gate_indices) and be non-decreasing")
        if gidx.shape[0] and gidx.min() < 0:
            raise ValueError("negative gate indices are not supported")
        ip_dtype = np.int32 if gidx.shape[0] <= _INT32_MAX else np.int64
        max_gate = int(gidx.max()) if gidx.shape[0] else -1
        self._dev = DeviceCSR(
            torch.from_numpy(indptr.astype(ip_dtype, copy=False)).to(dev),
            torch.from_numpy(gidx.astype(np.int32, copy=False)).to(dev),
            torch.from_numpy(wts.astype(np.float32, copy=False)).to(dev),
            max_gate)
        logger.info(f"Geometry resident on {dev}: {self._dev.nbytes() / 1e6:.1f} MB")
        return self._dev


def save_geometry(geometry: GridGeometry, filepath: str) -> None:
    """Write the nine-key ``.npz`` of ``radar_grid/geometry.py:105-116`` (deflate-compressed)."""
    np.savez_compressed(
        filepath,
        grid_shape=np.array(geometry.grid_shape),
        grid_limits_z=np.array(geometry.grid_limits[0]),
        grid_limits_y=np.array(geometry.grid_limits[1]),
        grid_limits_x=np.array(geometry.grid_limits[2]),
        indptr=geometry.indptr,
        gate_indices=geometry.gate_indices,
        weights=geometry.weights,
        toa=np.array([geometry.toa]),
        radar_altitude=np.array([geometry.radar_altitude]),
    )
    file_size_mb = os.path.getsize(filepath) / 1e6
    logger.info(f"Saved geometry to {filepath} ({file_size_mb:.1f} MB on disk)")


def load_geometry(filepath: str) -> GridGeometry:
    """Read a geometry ``.npz``; files without ``toa`` / ``radar_altitude`` default to ``inf`` / ``0.0``
    (``radar_grid/geometry.py:146-147``)."""
    with np.load(filepath) as data:
        geometry = GridGeometry(
            grid_shape=tuple(data["grid_shape"]),
            grid_limits=(tuple(data["grid_limits_z"]), tuple(data["grid_limits_y"]), tuple(data["grid_limits_x"])),
            indptr=data["indptr"],
            gate_indices=data["gate_indices"],
            weights=data["weights"],
            toa=float(data["toa"][0]) if "toa" in data else np.inf,
            radar_altitude=float(data["radar_altitude"][0]) if "radar_altitude" in data else 0.0,
        )
    logger.info(f"Loaded geometry: {geometry.memory_usage_mb():.1f} MB in memory, toa={geometry.toa}m")
    return geometry


# --------------------------------------------------------------------------------------------------------------------
# Sidecar of the device layout.  The reference's expensive precompute is a file (radar_grid/geometry.py:94-150) and that
# file -- the nine-key .npz above -- stays the interchange format.  What this build derives from it for large geometries
# (the compact copy: dictionaries + packed records) can be kept NEXT to it, so that a process that loads the .npz does
# not derive it again: an uncompressed .npz keyed by the sha256 of the reference arrays it was derived from, read with
# numpy.load(allow_pickle=False).  (A geometry built on the GPU from gate coordinates needs none of this: rebuilding the
# bench geometry takes 0.3 s of kernels, less than reading any file of its size.)
# --------------------------------------------------------------------------------------------------------------------
def _reference_arrays_digest(geometry: GridGeometry) -> str:
    import hashlib
    h = hashlib.sha256()
    h.update(repr((tuple(int(v) for v in geometry.grid_shape), _native.RG_COMPACT_LINES, _native.RG_COMPACT_ROTATION)).encode())
    for arr in (geometry.indptr, geometry.gate_indices, geometry.weights):
        a = np.ascontiguousarray(arr)
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(memoryview(a).cast("B"))
    return h.hexdigest()


def save_device_layout(geometry: GridGeometry, filepath: str, device=None) -> bool:
    """Write the compact copy of ``geometry`` (dictionaries, packed records or plain positions) as a sidecar ``.npz`` keyed by
    the digest of its reference arrays.  Returns ``False`` (nothing written) when the geometry has no compact copy."""
    compact = geometry.device_compact(device)
    if compact is None:
        return False
    csr = geometry.device_csr(device)
    compact.ensure_packed(csr)
    arrays = dict(key=np.frombuffer(_reference_arrays_digest(geometry).encode(), dtype=np.uint8),
                  grid_shape=np.array(compact.grid_shape, dtype=np.int64), dict_ptr=compact.dict_ptr.cpu().numpy(),
                  dict=compact.dict.cpu().numpy(), max_dict=np.array([compact.max_dict]), window_cap=np.array([compact.window_cap]),
                  chunk_pairs=compact.chunk_pairs.cpu().numpy(), chunk_counts=compact.chunk_counts.cpu().numpy())
    if compact.rec is not None:
        arrays.update(rec=compact.rec.cpu().numpy(), rec_ptr=compact.rec_ptr.cpu().numpy(),
                      rec_order=np.array([compact.rec_order]), w_base=np.array([compact.w_base], dtype=np.uint32),
                      rec_format=np.array([REC_FORMAT]))
    if compact.local_idx is not None:
        arrays["local_idx"] = compact.local_idx.cpu().numpy()
    np.savez(filepath, **arrays)
    written = os.fspath(filepath)
    written += "" if written.endswith(".npz") else ".npz"          # numpy.savez appends the suffix to a path without it
    logger.info(f"Saved device layout to {written} ({os.path.getsize(written) / 1e6:.1f} MB)")
    return True


def load_device_layout(geometry: GridGeometry, filepath: str, device=None) -> bool:
    """Attach the compact copy stored by :func:`save_device_layout` to ``geometry`` instead of deriving it again.  The
    sidecar is used only when its key matches the geometry's reference arrays (same CSR, same chunk layout); returns
    whether it was."""
    torch = _native.torch_mod()
    if not os.path.exists(filepath):
        return False
    with np.load(filepath, allow_pickle=False) as npz:
        if bytes(npz["key"]).decode() != _reference_arrays_digest(geometry):
            logger.warning(f"{filepath} was derived from another geometry: ignored")
            return False
        if "rec" in npz and ("rec_format" not in npz or int(npz["rec_format"][0]) != REC_FORMAT):
            logger.warning(f"{filepath} holds records in another coding than this build reads (no or another rec_format tag): "
                           "ignored, the device layout is derived again")
            return False
        data = {name: npz[name] for name in npz.files}
    reason = check_sidecar(ChunkLayout(geometry.grid_shape), data, geometry.n_pairs())     # before anything is uploaded
    if reason is not None:
        logger.warning(f"{filepath} does not hold the layout of this geometry ({reason}): ignored, the device layout is "
                       "derived again")
        return False
    csr = geometry.device_csr(device)
    dev = csr.indptr.device
    up = lambda name: torch.from_numpy(np.ascontiguousarray(data[name])).to(dev)       # noqa: E731
    compact = CompactCSR(up("local_idx") if "local_idx" in data else None, up("dict_ptr"), up("dict"), int(data["max_dict"][0]),
                         int(data["window_cap"][0]), tuple(int(v) for v in data["grid_shape"]), up("chunk_pairs"),
                         up("chunk_counts"))
    if "rec" in data:                                   # the row-end table is derived data: rebuilt, not stored
        compact.attach_records(up("rec"), up("rec_ptr"), int(data["rec_order"][0]), int(data["w_base"][0]), csr.indptr)
    geometry._compact = (csr, compact)
    logger.info(f"Device layout attached from {filepath}: {compact.nbytes() / 1e6:.1f} MB")
    return True
