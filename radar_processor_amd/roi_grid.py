"""Fused on-the-fly gridding (no CSR) -- ``rg_roi_grid_f32`` (csrc/rg_roi_grid.hip).

``compute_grid_geometry`` + ``apply_geometry`` in one kernel: for every voxel the neighbour search, the weights
(``radar_grid/compute.py:46-91``) and the masked weighted mean (``radar_grid/interpolate.py:69-104``) are
evaluated together and nothing but the output grid is written.  This is the path for grids whose CSR is too
large to be worth keeping; for repeated volumes on a moderate grid the CSR path (K1) is faster
because it amortises the search.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np

from . import _native
from .geometry_builder import WEIGHTINGS, RoiSearch
from .gridding import _stride_for


def pack_and_grid(dev, n_gates: int, fields: Sequence, masks: Optional[Sequence], shared_mask, out, out_shape, launch):
    """The one pack-and-grid loop of the CSR-free paths (lattice, mosaic, section).

    Validates the device-resident ``fields`` (float32) and ``masks`` / ``shared_mask`` (uint8, ``1`` = excluded, entries may
    be ``None``) for ``n_gates`` gates on ``dev`` and ``out`` for ``[F, *out_shape]`` (``None``: allocated here), then for
    every group of up to ``RG_MAX_FIELDS`` fields folds the masks into the packed buffer (``rg_pack_fields_f32``) and calls
    ``launch(packed, nf, stride, out_view, stream)`` -- ``out_view`` the group's ``[nf, prod(out_shape)]`` rows of ``out``.
    Raises ``ValueError`` before anything touches the device.  Returns ``out`` as ``[F, *out_shape]``."""
    torch = _native.torch_mod()
    n_fields = len(fields)
    if n_fields == 0:
        raise ValueError("no fields to grid")
    for i, f in enumerate(fields):
        if not (f.is_cuda and f.device == dev and f.dtype == torch.float32 and f.is_contiguous()
                and f.numel() == n_gates):
            raise ValueError(f"field {i}: expected a contiguous float32 tensor of {n_gates} gates on {dev}")
    if masks is None:
        masks = [None] * n_fields
    if len(masks) != n_fields:
        raise ValueError("masks must have one entry (tensor or None) per field")
    for i, m in enumerate(list(masks) + [shared_mask]):
        if m is not None and not (m.is_cuda and m.device == dev and m.dtype == torch.uint8 and m.is_contiguous()
                                  and m.numel() == n_gates):
            raise ValueError(f"mask {i}: expected a contiguous uint8 tensor of {n_gates} gates on {dev}")
    out_shape = tuple(int(n) for n in out_shape)
    n_out = int(np.prod(out_shape, dtype=np.int64))
    if out is not None and not (out.is_cuda and out.device == dev and out.dtype == torch.float32 and out.is_contiguous()
                                and out.numel() == n_fields * n_out):
        # the kernel writes n_fields * prod(out_shape) floats through a raw pointer: anything else is an out-of-bounds write
        raise ValueError(f"out must be a contiguous float32 tensor of shape [F, {', '.join(map(str, out_shape))}] on {dev}")
    lib = _native.load_library()
    if out is None:
        out = torch.empty((n_fields,) + out_shape, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        stream = _native.stream_ptr()
        for f0 in range(0, n_fields, _native.RG_MAX_FIELDS):
            group = list(range(f0, min(n_fields, f0 + _native.RG_MAX_FIELDS)))
            nf = len(group)
            stride = _stride_for(nf)
            packed = torch.empty(max(n_gates, 1) * stride, dtype=torch.float32, device=dev)
            fptrs = (ctypes.c_void_p * nf)(*[_native.ptr(fields[i]) for i in group])
            mptrs = (ctypes.c_void_p * nf)(*[_native.ptr(masks[i]) for i in group])
            _native.check(lib.rg_pack_fields_f32(nf, fptrs, mptrs, _native.ptr(shared_mask), n_gates, stride,
                                                 _native.ptr(packed), stream), "rg_pack_fields_f32")
            launch(packed, nf, stride, out.view(n_fields, n_out)[f0:f0 + nf], stream)
    return out.view((n_fields,) + out_shape)


def roi_grid_fields_device(search: RoiSearch, fields: Sequence, masks: Optional[Sequence] = None, shared_mask=None,
                           weighting: str = "barnes2", fill_value: float = np.nan, out=None):
    """Grid device-resident fields straight from the gates.  Arguments as ``grid_fields_device`` with a
    :class:`RoiSearch` (cell-sorted gates) in place of the CSR geometry.  Returns ``[F, nz, ny, nx]`` float32."""
    lib = _native.load_library()
    if weighting not in WEIGHTINGS and weighting != "closest":   # 'closest' = single nearest gate (fused path only)
        raise ValueError(f"Unknown weighting function: {weighting}")
    fill = float(np.float32(fill_value))

    def launch(packed, nf, stride, out_view, stream):
        _native.check(lib.rg_roi_grid_f32(*search.search_args(), _native.WEIGHTINGS[weighting], _native.ptr(packed), nf,
                                          stride, fill, _native.ptr(out_view), stream), "rg_roi_grid_f32")
    return pack_and_grid(search.dev, search.n_gates, fields, masks, shared_mask, out, search.grid_shape, launch)
