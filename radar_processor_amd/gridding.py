"""Field gridding through a precomputed geometry -- mirror of ``radar_grid/interpolate.py``
(``apply_geometry`` :15-104, ``apply_geometry_multi`` :107-142), executed by the HIP kernel
``rg_csr_apply_f32`` (csrc/rg_csr_apply.hip).

Two layers:

* :func:`apply_geometry` / :func:`apply_geometry_multi` keep the reference signatures (NumPy masked arrays in,
  float32 ``ndarray`` of ``geometry.grid_shape`` out).  They stage the inputs into HBM, run the kernels and
  copy the grid back; the geometry itself is uploaded once and cached on the ``GridGeometry`` object.
* :func:`grid_fields_device` is the device-resident form the batch driver and the benchmark use: field
  tensors already in HBM in, grid tensor in HBM out, nothing crosses PCIe.

All fields handed to one call are gridded by ONE pass over the CSR (the reference re-reads the CSR per field,
interpolate.py:137-140): the mask of every field is folded into its values and the fields are interleaved
gate-major, so each (voxel, gate) pair costs a single gather.  Passes over a large geometry (50 M pairs and up) run
through a compact device copy of the CSR, built the first time the geometry grids something (16-bit positions in a
per-chunk gate dictionary, the chunk's field values staged in LDS, positions and weights packed three pairs to a 16-byte
record where the weights allow: ``rg_csr_compact_apply_packed_f32`` / ``rg_csr_compact_apply_f32``) -- the same values to
float32 rounding, 35-50 % less time.
"""
from __future__ import annotations

import ctypes
import logging
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _native, pass_policy
from .gate_filters import GateFilter
from .grid_geometry import GridGeometry
from .grid_products import EFFECTIVE_RADIUS_FACTOR

logger = logging.getLogger("radar_grid.interpolate")


def _stride_for(n_fields: int) -> int:
    return 1 if n_fields == 1 else 2 if n_fields == 2 else 4 if n_fields <= 4 else 8


def _coerce_filters(additional_filters) -> List[GateFilter]:
    """``None`` -> ``[]``, a bare filter -> ``[gf]``, a list stays, anything else is a ValueError
    (``interpolate.py:50-56``)."""
    if isinstance(additional_filters, list):
        return additional_filters
    if additional_filters is None:
        return []
    if isinstance(additional_filters, GateFilter):
        return [additional_filters]
    raise ValueError("additional_filters must be a list of GateFilter objects")


def _host_field(field_data, filters: Sequence[GateFilter]):
    """float32 values + merged exclusion mask (``interpolate.py:59-64``).

    The reference indexes ``np.ma.getmask(field)`` and therefore crashes on inputs without a full mask
     unless a filter happens to broadcast it; here a missing mask simply means "nothing masked",
    which is also what the reference computes whenever it does not crash.
    """
    values = np.ascontiguousarray(np.ma.getdata(field_data), dtype=np.float32).ravel()
    mask = np.ma.getmaskarray(field_data).ravel()
    for gf in filters:
        mask = mask | gf.gate_excluded
    return values, np.ascontiguousarray(mask, dtype=np.uint8)


class CsrGridder:
    """Persistent device buffers + launches for gridding field groups of a fixed size through one geometry.

    Holds the packed-field staging buffer so that repeated volumes cost no allocation, and exposes the two
    stages separately (``pack`` = mask fold + interleave, ``apply`` = the CSR pass) so that callers can time
    or graph-capture them.  All launches go to torch's current stream.
    """

    def __init__(self, geometry: GridGeometry, n_gates: int, n_fields: int, device=None, compact: bool = False,
                 tile: int = 0, packed: bool = True):
        """``compact``: run the pass through the compact device copy of the CSR (built and cached on the geometry the
        first time) when the geometry allows one and its LDS window for this field count covers (nearly) all pairs:
        ``rg_csr_compact_apply_packed_f32`` (row-wise kernel over the packed records; agrees with ``rg_csr_apply_f32`` to
        float32 rounding) for 1-8 fields when the weights are codable and ``packed`` is set, ``rg_csr_compact_apply_f32``
        (tile kernel; agrees bit for bit) otherwise.  ``tile``: diagnostic override -- 128...512 the pipeline tile of the
        tile kernels (non-default values change the order of the float32 adds), 384 also selects the tile kernel over
        the packed records, 2000 + h the lane split of the row-wise kernel."""
        torch = _native.torch_mod()
        self.lib = _native.load_library()
        if not 1 <= n_fields <= _native.RG_MAX_FIELDS:
            raise ValueError(f"n_fields must be in 1..{_native.RG_MAX_FIELDS}")
        self.dev = _native.canonical_device(device)
        self.csr = geometry.device_csr(self.dev)
        self.n_gates = int(n_gates)
        self.n_fields = int(n_fields)
        self.stride = _stride_for(n_fields)
        self.tile = int(tile)
        self.grid_shape = tuple(int(s) for s in geometry.grid_shape)
        self.n_vox = int(np.prod(self.grid_shape))
        if self.n_vox != self.csr.n_vox:
            raise ValueError(f"grid_shape {self.grid_shape} does not match the geometry's {self.csr.n_vox} rows")
        if self.csr.max_gate >= self.n_gates:
            # the reference's fancy index (interpolate.py:74) raises the same way
            raise IndexError(f"index {self.csr.max_gate} is out of bounds for axis 0 with size {self.n_gates}")
        self.packed = torch.empty(max(self.n_gates, 1) * self.stride, dtype=torch.float32, device=self.dev)
        self._columns_ws = None
        # which kernel, with which window: pass_policy.choose_pass.  The attributes stay plain: apply() dispatches from them
        csr, copy_of = _policy_facts(geometry, self.dev)
        choice = pass_policy.choose_pass(self.n_fields, csr.n_pairs, csr.gate_indices is not None, csr.weights is not None,
                                         compact, packed, copy_of)
        self.compact = choice.copy.compact if choice.use_compact else None
        self.window = choice.window
        self.packed_stream = choice.packed_stream

    def _check_fields(self, fields, masks, shared_mask):
        torch = _native.torch_mod()
        if len(fields) != self.n_fields:
            raise ValueError(f"expected {self.n_fields} fields, got {len(fields)}")
        for i, f in enumerate(fields):
            if not (f.is_cuda and f.device == self.packed.device and f.dtype == torch.float32 and f.is_contiguous()
                    and f.numel() == self.n_gates):
                raise ValueError(f"field {i}: expected a contiguous cuda float32 tensor of {self.n_gates} gates "
                                 f"on {self.packed.device}")
        if len(masks) != self.n_fields:
            raise ValueError("masks must have one entry (tensor or None) per field")
        for i, m in enumerate(list(masks) + [shared_mask]):
            if m is not None and not (m.is_cuda and m.device == self.packed.device and m.dtype == torch.uint8
                                      and m.is_contiguous() and m.numel() == self.n_gates):
                raise ValueError(f"mask {i}: expected a contiguous cuda uint8 tensor of {self.n_gates} gates")

    def pack(self, fields: Sequence, masks: Optional[Sequence] = None, shared_mask=None) -> None:
        """``rg_pack_fields_f32``: fold every field's exclusion mask into its values, interleave gate-major."""
        masks = [None] * self.n_fields if masks is None else list(masks)
        self._check_fields(fields, masks, shared_mask)
        nf = self.n_fields
        fptrs = (ctypes.c_void_p * nf)(*[_native.ptr(f) for f in fields])
        mptrs = (ctypes.c_void_p * nf)(*[_native.ptr(m) for m in masks])
        _native.check(self.lib.rg_pack_fields_f32(nf, fptrs, mptrs, _native.ptr(shared_mask), self.n_gates, self.stride,
                                                  _native.ptr(self.packed), _native.stream_ptr()), "rg_pack_fields_f32")

    def apply(self, out, fill_value: float = np.nan) -> None:
        """One pass over the CSR for all packed fields -> ``out[F, n_vox]`` (``rg_csr_compact_apply_packed_f32`` /
        ``rg_csr_compact_apply_f32`` through the compact copy, ``rg_csr_apply_f32`` otherwise)."""
        csr = self.csr
        nz, ny, nx = self.grid_shape
        kernel, tile = pass_policy.tile_override(self.tile, self.packed_stream, self.compact is not None,
                                                 csr.weights is not None)
        if kernel == pass_policy.KERNEL_ROWWISE:
            _native.check(self.lib.rg_csr_compact_apply_packed_f32_ex(
                *self._stream_args(fill_value), _native.ptr(out), self.window, tile, _native.ptr(self.compact.row_end16),
                _native.stream_ptr()), kernel)
        elif kernel == pass_policy.KERNEL_TILE:
            c = self.compact
            _native.check(self.lib.rg_csr_compact_apply_f32(
                _native.ptr(csr.indptr), int(csr.is_i64), _native.ptr(c.local_idx), _native.ptr(csr.weights),
                _native.ptr(c.dict_ptr), _native.ptr(c.dict), self.n_vox, csr.n_pairs, nx, ny, _native.ptr(self.packed),
                self.n_fields, self.stride, self.n_gates, float(np.float32(fill_value)), _native.ptr(out), self.window,
                tile, _native.stream_ptr()), kernel)
        else:
            _native.check(self.lib.rg_csr_apply_f32_ex(
                _native.ptr(csr.indptr), int(csr.is_i64), _native.ptr(csr.gate_indices), _native.ptr(csr.weights),
                self.n_vox, csr.n_pairs, nx, _native.ptr(self.packed), self.n_fields, self.stride, self.n_gates,
                float(np.float32(fill_value)), _native.ptr(out), tile, _native.stream_ptr()), kernel)

    def _stream_args(self, fill_value):
        """The 17 leading arguments ``rg_csr_compact_apply_packed_f32``, ``_columns_f32`` and ``_planes_f32`` share with their
        ``_ex`` variants, which :meth:`apply`, :meth:`apply_columns` and :meth:`apply_planes` call with the compact copy's
        row-end table (a null pointer where it has none: every segment then reads the row pointers)."""
        csr, c = self.csr, self.compact
        nz, ny, nx = self.grid_shape
        return (_native.ptr(csr.indptr), int(csr.is_i64), _native.ptr(c.rec), _native.ptr(c.rec_ptr), c.rec_order, c.w_base,
                _native.ptr(c.dict_ptr), _native.ptr(c.dict), self.n_vox, csr.n_pairs, nx, ny, _native.ptr(self.packed),
                self.n_fields, self.stride, self.n_gates, float(np.float32(fill_value)))

    def _columns_workspace(self, nbytes: int):
        """The grow-only device workspace of the column and planes modes (partial planes of the level pieces)."""
        torch = _native.torch_mod()
        ws = self._columns_ws
        if ws is None or ws.numel() < nbytes:
            ws = self._columns_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        return ws

    # ---- column mode of the row-wise kernel (rg_csr_compact_apply_columns_f32) ----------------------------------------
    @property
    def has_columns_kernel(self) -> bool:
        """The column mode of the row-wise kernel reads the packed records: 1-4 fields, codable weights."""
        return pass_policy.has_columns_kernel(self.compact is not None, self.packed_stream, self.n_fields)

    def _column_plan(self, z_pieces: int):
        """``(z_pieces, order tensor)`` for this geometry: enough workgroups to fill the chip (a workgroup is one column
        of chunks, or one of ``z_pieces`` level ranges of it), listed heaviest first -- workgroups are handed out in
        ``blockIdx`` order as slots free up, so starting the long columns first is what keeps the tail short (greedy
        longest-processing-time scheduling).  Cached on the compact copy."""
        torch = _native.torch_mod()
        c = self.compact
        nz = self.grid_shape[0]
        n_cols = c.chunks.nsx * c.chunks.nyg
        if z_pieces <= 0:
            z_pieces = pass_policy.column_pieces(nz, n_cols)
        z_pieces = max(1, min(int(z_pieces), nz))
        cache = c._column_orders
        order = cache.get(z_pieces)
        if order is None:
            if c.chunk_pairs is not None and c.chunk_pairs.numel() == c.chunks.n_chunks:
                weight = c.chunks.column_weights(c.chunk_pairs, z_pieces)
                order = torch.argsort(weight, descending=True, stable=True).to(torch.int32)
            else:
                order = False                                        # no statistics: identity order
            cache[z_pieces] = order
        return z_pieces, (None if order is False else order)

    def apply_columns(self, out=None, fill_value: float = np.nan, level_planes=None, keep_lo: int = 0, col_max=None,
                      col_arg=None, col_window=None, z_pieces: int = 0, lanes_hint: int = 0, ordered: bool = True) -> None:
        """One pass of ``rg_csr_compact_apply_columns_f32`` over the packed records (the row-wise kernel with every workgroup
        walking the levels of one column of chunks): ``out`` ``[F, n_vox]`` receives the same bits as :meth:`apply` with the
        row-wise kernel, or is ``None`` when only 2-D products are wanted -- ``level_planes`` ``[F, n_keep, ny, nx]``
        (planes ``keep_lo ..`` of every grid), ``col_max`` / ``col_arg`` ``[F, ny, nx]`` (``column_argmax`` over the level
        window ``col_window = (lo, hi)``, default all levels)."""
        if not self.has_columns_kernel:
            raise _native.NativeError("the column mode needs the packed records (1-4 fields, codable weights)")
        nz, ny, nx = self.grid_shape
        n_keep = 0 if level_planes is None else int(level_planes.shape[1])
        lo, hi = (0, nz - 1) if col_window is None else (int(col_window[0]), int(col_window[1]))
        pieces, order = self._column_plan(z_pieces)
        if not ordered:
            order = None
        ws = None
        if col_max is not None and pieces > 1:
            ws = self._columns_workspace(int(self.lib.rg_csr_columns_workspace_bytes(ny, nx, self.n_fields, pieces)))
        _native.check(self.lib.rg_csr_compact_apply_columns_f32_ex(
            *self._stream_args(fill_value), _native.ptr(out),
            _native.ptr(level_planes), int(keep_lo), n_keep, _native.ptr(col_max), _native.ptr(col_arg), lo, hi, self.window,
            pieces, _native.ptr(order), _native.ptr(ws), 0 if ws is None else int(ws.numel()), int(lanes_hint),
            _native.ptr(self.compact.row_end16), _native.stream_ptr()), "rg_csr_compact_apply_columns_f32")

    def columns_bytes(self, store_grid: bool, n_keep: int = 0, colmax: bool = False) -> Optional[int]:
        """Bytes one ``apply_columns`` launch must move: the compact kernel's, minus the grids that are not stored, plus the
        kept planes and the (max, arg) planes."""
        base = self.compact_bytes(grid_mode=False)
        if base is None:
            return None
        nz, ny, nx = self.grid_shape
        return (base - (0 if store_grid else self.n_fields * 4 * self.n_vox)
                + self.n_fields * 4 * ny * nx * (int(n_keep) + (2 if colmax else 0)))

    def apply_planes(self, out=None, fill_value: float = np.nan, level_planes=None, keep_lo: int = 0, col_max=None, col_arg=None,
                     col_min=None, col_mean=None, col_window=None, sel_levels: Sequence = (), sel_samples=None,
                     z_pieces: int = 0, lanes_hint: int = 0, ordered: bool = True) -> None:
        """One pass of ``rg_csr_compact_apply_planes_f32``: :meth:`apply_columns` with the wider epilogue -- next to ``out`` /
        ``level_planes`` / ``col_max`` / ``col_arg`` (same meaning), ``col_min`` and ``col_mean`` ``[F, ny, nx]``
        (``column_min`` / ``column_mean`` over ``col_window``) and up to ``RG_MAX_SEL_PLANES`` per-pixel level selections
        (``sel_levels``: int32 ``[ny, nx]`` tensors from ``grid_products.ppi_plan``) whose levels land in ``sel_samples``
        ``[F, n_sel, 2, ny, nx]`` for ``grid_products.ppi_finish``.  ``col_mean`` takes one level piece (its float32 running
        sum cannot be split): ``z_pieces`` is then 1."""
        if not self.has_columns_kernel:
            raise _native.NativeError("the planes mode needs the packed records (1-4 fields, codable weights)")
        nz, ny, nx = self.grid_shape
        n_sel = len(sel_levels)
        if n_sel > _native.RG_MAX_SEL_PLANES:
            raise ValueError(f"at most {_native.RG_MAX_SEL_PLANES} level selections per launch, got {n_sel}")
        lo, hi = (0, nz - 1) if col_window is None else (int(col_window[0]), int(col_window[1]))
        pieces, order = self._column_plan(1 if col_mean is not None else z_pieces)
        if not ordered:
            order = None
        ws = None
        if (col_max is not None or col_min is not None) and pieces > 1:
            ws = self._columns_workspace(int(self.lib.rg_csr_planes_workspace_bytes(
                ny, nx, self.n_fields, pieces, int(col_max is not None), int(col_min is not None))))
        req = _native.PlaneRequest(out=_native.ptr(out), level_planes=_native.ptr(level_planes), keep_lo=int(keep_lo),
                                   n_keep=0 if level_planes is None else int(level_planes.shape[1]),
                                   col_max=_native.ptr(col_max), col_arg=_native.ptr(col_arg), col_min=_native.ptr(col_min),
                                   col_mean=_native.ptr(col_mean), col_lo=lo, col_hi=hi, n_sel=n_sel,
                                   sel_samples=_native.ptr(sel_samples))
        for k, sel in enumerate(sel_levels):
            req.sel_levels[k] = _native.ptr(sel)
        _native.check(self.lib.rg_csr_compact_apply_planes_f32_ex(
            *self._stream_args(fill_value), ctypes.byref(req), self.window, pieces,
            _native.ptr(order), _native.ptr(ws), 0 if ws is None else int(ws.numel()), int(lanes_hint),
            _native.ptr(self.compact.row_end16), _native.stream_ptr()), "rg_csr_compact_apply_planes_f32")

    def planes_bytes(self, store_grid: bool, n_keep: int = 0, colmax: bool = False, argmax: bool = False,
                     colmin: bool = False, colmean: bool = False, n_sel: int = 0) -> Optional[int]:
        """Bytes one ``apply_planes`` launch must move: the compact kernel's, minus the grids that are not stored, plus the
        kept, max / arg / min / mean planes, the selection words read and (at most) two samples per selection written."""
        base = self.compact_bytes(grid_mode=False)
        if base is None:
            return None
        nz, ny, nx = self.grid_shape
        per_field = int(n_keep) + int(bool(colmax)) + int(bool(argmax)) + int(bool(colmin)) + int(bool(colmean)) + 2 * int(n_sel)
        return (base - (0 if store_grid else self.n_fields * 4 * self.n_vox) + self.n_fields * 4 * ny * nx * per_field
                + 4 * ny * nx * int(n_sel))

    def algorithmic_bytes(self) -> int:
        """Bytes one ``apply`` launch must move: index + weight per pair, the row pointers,
        each field's values + mask once, each output grid once."""
        csr = self.csr
        ip = 8 if csr.is_i64 else 4
        return 8 * csr.n_pairs + ip * (self.n_vox + 1) + self.n_fields * (5 * self.n_gates + 4 * self.n_vox)

    def settle_records(self, tries: int = 3, probe_launches: int = 3, out=None):
        """Placement settling of the packed record array -- part of the one-off geometry build, like the reference's
        precompute (``radar_grid/compute.py:106-284`` runs once per scan strategy, ``apply_geometry`` thousands of times).

        On this part the 1.4 % of its traffic the gridding kernel WRITES costs 5-15 % of the launch depending on where the
        driver happened to place the 44 GB it READS (EXPERIMENTS.md: thirty + twenty processes in two clusters, the placement
        decided per allocation, nothing on the kernel's side moves it).  So: copy the records into ``tries - 1`` further
        allocations, time ``probe_launches`` launches of this gridder's own kernel through each (the fields are whatever
        ``packed`` holds; values do not matter to the timing), keep the fastest placement and free the others.  Needs
        ``tries`` x the record bytes of free HBM for a moment (skipped otherwise); nothing about the results changes -- the
        same records, the same kernel, the same bits.  Returns ``{"tries", "probe_ms", "kept"}`` or ``None`` when it did
        not run."""
        torch = _native.torch_mod()
        c = self.compact
        if c is None or not self.packed_stream or tries <= 1 or c.rec is None or c.rec.numel() == 0:
            return None
        nbytes = int(c.rec.numel()) * c.rec.element_size()
        free_b, _ = torch.cuda.mem_get_info(self.dev)
        if not pass_policy.settle_copies_fit(nbytes, tries, 4 * self.n_fields * self.n_vox, free_b):
            return None
        with torch.cuda.device(self.dev):
            if out is None:
                out = torch.empty((self.n_fields, self.n_vox), dtype=torch.float32, device=self.dev)
            candidates = [c.rec] + [torch.empty_like(c.rec).copy_(c.rec) for _ in range(tries - 1)]      # all alive at once:
            probe_ms = []                                                                                # distinct placements
            for cand in candidates:
                c.rec = cand
                self.apply(out)                                         # warm-up through this placement
                times = []
                for _ in range(probe_launches):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    self.apply(out)
                    e1.record()
                    e1.synchronize()
                    times.append(e0.elapsed_time(e1))
                probe_ms.append(round(float(np.median(times)), 4))
            kept = int(np.argmin(probe_ms))
            c.rec = candidates[kept]
            del candidates, cand
            torch.cuda.empty_cache()                                    # hand the losers' memory back to the driver
        logger.info(f"Record placement settled: probe ms {probe_ms}, kept allocation {kept}")
        return {"tries": tries, "probe_ms": probe_ms, "kept": kept}

    def compact_bytes(self, grid_mode: bool = True) -> Optional[int]:
        """Bytes one launch of the compact kernel must move: the packed records as stored (or 16-bit position + weight per
        pair), the dictionaries and their offsets, the row pointers -- through the records: what the row-wise kernel reads of
        them, ``CompactCSR.row_pointer_bytes`` (2-byte row ends where a segment's span fits, nothing for a chunk without a
        pair) --, every field once, every grid once (``None`` without a compact copy)."""
        if self.compact is None:
            return None
        csr, c = self.csr, self.compact
        ip = 8 if csr.is_i64 else 4
        if self.packed_stream:      # the records' 16-byte units (14-byte records where the chunk is dense) + one offset per segment
            stream = 16 * int(c.rec.shape[0]) + 8 * int(c.rec_ptr.numel())
            rows = c.row_pointer_bytes(csr.indptr, grid_mode)      # the column and planes modes leave no chunk early
        else:
            stream = 6 * csr.n_pairs
            rows = ip * (self.n_vox + 1)
        return (stream + 4 * c.n_dict + 8 * int(c.dict_ptr.numel()) + rows
                + self.n_fields * (5 * self.n_gates + 4 * self.n_vox))


def _policy_facts(geometry: GridGeometry, dev):
    """``(device CSR, copy_of)``: what ``pass_policy`` asks about ``geometry`` on ``dev``.  ``copy_of()`` builds (once) the
    compact copy and yields its ``pass_policy.CopyFacts``, or ``None`` when the geometry cannot be compacted."""
    csr = geometry.device_csr(dev)

    def copy_of():
        c = geometry.device_compact(dev)
        return None if c is None else pass_policy.CopyFacts(c.window_cap, c.fallback_fraction, lambda: c.ensure_packed(csr), c)
    return csr, copy_of


def _use_compact(geometry: GridGeometry, dev) -> bool:
    """``pass_policy.use_compact`` for ``geometry`` on ``dev``: do its passes run through the compact copy of its CSR?
    (``GridGeometry.device_compact()`` builds the copy explicitly ahead of time.)"""
    csr = geometry.device_csr(dev)
    cached = getattr(geometry, "_compact", None)
    state = (cached[1] is not None) if (cached is not None and cached[0] is csr) else None
    return pass_policy.use_compact(state, csr.n_pairs, lambda: _native.torch_mod().cuda.mem_get_info(dev)[0])


def _pass_size(policy, geometry: GridGeometry, dev, use_compact: bool) -> int:
    csr, copy_of = _policy_facts(geometry, dev)
    return policy(csr.n_pairs, csr.weights is not None, use_compact, copy_of)


def fields_per_pass(geometry: GridGeometry, device=None) -> int:
    """How many fields (or field-volumes of a batch) ``grid_fields_device`` fuses into one pass over this geometry on
    ``device`` (builds the device copy if it does not exist yet): ``pass_policy.fields_per_pass``."""
    dev = _native.canonical_device(device)
    return _pass_size(pass_policy.fields_per_pass, geometry, dev, _use_compact(geometry, dev))


def volumes_per_pass_cap(geometry: GridGeometry, device=None) -> int:
    """Field-volumes of a batch one pass should fuse (``batch.VolumeBatch``): ``pass_policy.volumes_per_pass_cap``."""
    dev = _native.canonical_device(device)
    return _pass_size(pass_policy.volumes_per_pass_cap, geometry, dev, _use_compact(geometry, dev))


def _cached_gridder(geometry: GridGeometry, n_gates: int, n_fields: int, dev, compact: bool) -> "CsrGridder":
    """One :class:`CsrGridder` (and its packed-field staging buffer) per (device CSR, gate count, field count, kernel)
    of a geometry, kept on the geometry object: repeated ``apply_geometry`` calls allocate nothing.  The cache dies with
    the device copy (``GridGeometry.invalidate_device`` / attribute assignment)."""
    csr = geometry.device_csr(dev)
    cache = geometry.__dict__.setdefault("_gridders", {})
    key = (id(csr), int(n_gates), int(n_fields), bool(compact))
    gridder = cache.get(key)
    if gridder is None or gridder.csr is not csr:
        if len(cache) >= 8:                 # a handful of shapes per geometry is the norm; never grow without bound
            cache.clear()
        gridder = cache[key] = CsrGridder(geometry, n_gates, n_fields, device=dev, compact=compact)
    return gridder


def _pass_groups(geometry: GridGeometry, n_gates: int, n_fields: int, dev, cap: Optional[int] = None):
    """Cut ``n_fields`` fields into the passes ``pass_policy`` chooses for ``geometry`` on ``dev`` (at most ``cap`` fields
    each): yields ``(f0, f1, gridder)`` per pass, the gridder from :func:`_cached_gridder`."""
    use_compact = _use_compact(geometry, dev)
    per_pass = _pass_size(pass_policy.fields_per_pass, geometry, dev, use_compact)
    if cap is not None:
        per_pass = min(per_pass, cap)
    for f0 in range(0, n_fields, per_pass):
        f1 = min(n_fields, f0 + per_pass)
        yield f0, f1, _cached_gridder(geometry, n_gates, f1 - f0, dev, compact=use_compact)


def grid_fields_device(geometry: GridGeometry, fields: Sequence, masks: Optional[Sequence] = None,
                       shared_mask=None, fill_value: float = np.nan, out=None):
    """Grid ``len(fields)`` device-resident fields with one CSR pass per group of up to 8.

    Parameters
    ----------
    fields : sequence of cuda float32 tensors ``[G]``
    masks : optional sequence (same length) of uint8 tensors ``[G]`` or ``None`` (``1`` = gate excluded)
    shared_mask : optional uint8 tensor OR-ed into every field's mask (e.g. one QC GateFilter for all)
    out : optional float32 tensor ``[len(fields), nz, ny, nx]`` to write into

    Returns the ``[F, nz, ny, nx]`` float32 tensor (device).
    """
    torch = _native.torch_mod()
    n_fields = len(fields)
    if n_fields == 0:
        raise ValueError("no fields to grid")
    dev = fields[0].device
    if dev.type != "cuda":
        raise _native.NativeUnavailable("grid_fields_device needs device-resident (cuda) tensors")
    if masks is None:
        masks = [None] * n_fields
    if len(masks) != n_fields:
        raise ValueError("masks must have one entry (tensor or None) per field")
    nz, ny, nx = (int(s) for s in geometry.grid_shape)
    n_vox = nz * ny * nx
    if out is None:
        out = torch.empty((n_fields, nz, ny, nx), dtype=torch.float32, device=dev)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == n_fields * n_vox):
        raise ValueError("out must be a contiguous cuda float32 tensor of shape [F, nz, ny, nx]")
    n_gates = int(fields[0].numel())
    with torch.cuda.device(dev):
        for f0, f1, gridder in _pass_groups(geometry, n_gates, n_fields, dev):
            gridder.pack(fields[f0:f1], masks[f0:f1], shared_mask)
            gridder.apply(out.view(n_fields, n_vox)[f0:f1], fill_value)
    return out.view(n_fields, nz, ny, nx)


class PlaneProducts:
    """The 2-D products a products-only pass keeps of every gridded field (``grid_products_device``,
    ``batch.VolumeBatch.grid_shard(products=PlaneProducts(...))``): the column maximum over a level window
    (``radar_grid/products.py:420-490``; same window arguments as ``column_max``), optionally the level that attains it
    (``column_argmax``), the column minimum / mean over the same window (``column_min`` :493-535, ``column_mean`` :538-580),
    CAPPIs at the given altitudes (``products.py:317-415``) and constant-elevation PPIs at the given angles (``ppi``,
    ``constant_elevation_ppi`` :168-314).  With these and nothing else wanted, the 3-D grid never has to exist in HBM: the
    gridding kernel, walking grid columns, keeps the running maximum / minimum / sum in registers and stores only the levels
    the CAPPIs blend and the levels each PPI pixel reads.

    The column PROFILE products -- ``echo_top`` / ``echo_base`` heights at the given thresholds and ``vil``
    (``grid_products.column_profile``, over the same level window) -- are computed from the stored grid by
    ``rg_column_profile_f32``: the gridding kernels' epilogues do not produce them, so a request that holds one grids, then
    reduces, and ``fused=True`` together with one is refused."""

    def __init__(self, colmax: bool = True, argmax: bool = True, cappi: Sequence[float] = (), interpolation: str = "linear",
                 z_min_idx: Optional[int] = None, z_max_idx: Optional[int] = None, z_min_alt: Optional[float] = None,
                 z_max_alt: Optional[float] = None, fused: Optional[bool] = None, colmin: bool = False, colmean: bool = False,
                 ppi: Sequence[float] = (), ppi_interpolation: str = "linear", earth_curvature: bool = True,
                 ke: float = EFFECTIVE_RADIUS_FACTOR, echo_top: Sequence[float] = (), echo_base: Sequence[float] = (),
                 vil: bool = False, vil_max_dbz: float = 56.0, profile_interpolation: str = "linear"):
        """``fused``: ``True`` = take the planes out of the gridding kernel (no 3-D grid in HBM: the memory-saving way),
        ``False`` and ``None`` (the default) = grid, then reduce with the separate kernels: measured, the epilogue saves
        memory, not time (``pass_policy.run_fused``).  The same planes either way, bit for bit.  ``ppi``: elevation angles (degrees); ``ppi_interpolation`` / ``earth_curvature`` /
        ``ke`` as in ``constant_elevation_ppi`` ('linear' planes are float64, 'nearest' float32).  ``echo_top`` /
        ``echo_base``: thresholds; ``vil`` with ``vil_max_dbz``; ``profile_interpolation`` as ``column_profile``'s
        ``interpolation``."""
        from .grid_products import check_profile_request
        if interpolation not in ("linear", "nearest"):
            raise ValueError(f"Unknown interpolation method: {interpolation}")
        if ppi_interpolation not in ("linear", "nearest"):
            raise ValueError(f"Unknown interpolation method: {ppi_interpolation}")
        self.colmax = bool(colmax or argmax)
        self.argmax = bool(argmax)
        self.cappi = tuple(float(a) for a in cappi)
        self.interpolation = interpolation
        self.window = (z_min_idx, z_max_idx, z_min_alt, z_max_alt)
        self.fused = fused
        self.colmin = bool(colmin)
        self.colmean = bool(colmean)
        self.ppi = tuple(float(e) for e in ppi)
        self.ppi_interpolation = ppi_interpolation
        self.earth_curvature = bool(earth_curvature)
        self.ke = float(ke)
        self.echo_top, self.echo_base = check_profile_request(echo_top, echo_base, vil, vil_max_dbz, profile_interpolation)
        self.vil = bool(vil)
        self.vil_max_dbz = float(vil_max_dbz)
        self.profile_interpolation = profile_interpolation
        if fused and self.profile:
            raise ValueError("fused=True cannot produce echo_top / echo_base / vil: the gridding kernels' epilogues do not "
                             "compute them (leave fused unset: grid, then reduce)")

    @property
    def columns(self) -> bool:
        """Any product over the level window."""
        return self.colmax or self.colmin or self.colmean

    @property
    def profile(self) -> bool:
        """Any column profile product (echo top / base, VIL): computed from the stored grid only."""
        return bool(self.echo_top or self.echo_base or self.vil)

    @property
    def needs_planes_mode(self) -> bool:
        """Products the column mode's epilogue (``rg_csr_compact_apply_columns_f32``) does not compute: the fused pass runs
        ``rg_csr_compact_apply_planes_f32`` instead."""
        return self.colmin or self.colmean or bool(self.ppi)


def _to_host(t) -> np.ndarray:
    """Device -> NumPy through a page-locked staging tensor (about twice the rate of a pageable copy; the
    640 MB grid download dominates the NumPy-in / NumPy-out path).  The array owns its buffer."""
    torch = _native.torch_mod()
    try:
        host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    except RuntimeError:        # no pinned memory available: plain copy
        return t.cpu().numpy()
    host.copy_(t, non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    return host.numpy()


def apply_geometry(geometry: GridGeometry, field_data: np.ndarray,
                   additional_filters: Optional[List[GateFilter]] = None,
                   fill_value: float = np.nan) -> np.ndarray:
    """Weighted-mean gridding of one field (``radar_grid/interpolate.py:15-104``).

    ``field_data``: flattened (masked) field, shape ``(n_gates,)``; masked gates and gates excluded by any of
    ``additional_filters`` contribute to neither sum; voxels without a positive weight sum get ``fill_value``.
    Returns a float32 array of shape ``geometry.grid_shape``.
    """
    filters = _coerce_filters(additional_filters)
    values, mask = _host_field(field_data, filters)
    torch = _native.torch_mod()
    dev = _native.device()
    f_t = torch.from_numpy(values).to(dev)
    m_t = torch.from_numpy(mask).to(dev) if mask.any() else None
    grid = grid_fields_device(geometry, [f_t], [m_t], fill_value=fill_value)
    return _to_host(grid[0]).reshape(geometry.grid_shape)


def apply_geometry_multi(geometry: GridGeometry, fields: Dict[str, np.ndarray],
                         additional_filters: Optional[Dict[str, List[GateFilter]]] = None,
                         fill_value: float = np.nan) -> Dict[str, np.ndarray]:
    """Grid several fields (``radar_grid/interpolate.py:107-142``) -- one CSR pass for all of them.

    ``additional_filters`` maps a field name to its filter list (a missing name means no filters).
    """
    if additional_filters is None:
        additional_filters = {}
    names = list(fields.keys())
    if not names:
        return {}
    torch = _native.torch_mod()
    dev = _native.device()
    f_ts, m_ts = [], []
    for name in names:
        values, mask = _host_field(fields[name], _coerce_filters(additional_filters.get(name, None)))
        f_ts.append(torch.from_numpy(values).to(dev))
        m_ts.append(torch.from_numpy(mask).to(dev) if mask.any() else None)
    grid = _to_host(grid_fields_device(geometry, f_ts, m_ts, fill_value=fill_value))
    return {name: grid[i].reshape(geometry.grid_shape) for i, name in enumerate(names)}
