"""Connected echo regions on the device: labelling, the cell table, despeckling (include/radargrid_hip.h, "Connected echo
regions"; kernels in csrc/rg_components.hip).

Two uses of one kernel family:

* **despeckle** -- remove echo regions smaller than ``min_size`` pixels from product planes before they are coloured, or from
  one sweep ``[n_rays, n_gates]`` with ``wrap_rows=True`` (the azimuth axis wraps; PyART's ``despeckle_field``), whose
  ``uint8`` mask is what the gridders' ``masks`` arguments take;
* **storm cells** -- the connected regions at or above a threshold with area, bounding box, centroid, peak and peak position.

A pixel is foreground iff ``threshold <= v <= upper`` in float32 and ``mask`` is zero there; NaN never is.  Cells are numbered
from 1 per plane in raster order of their first pixel (``scipy.ndimage.label``'s numbering).  The device functions take and
return tensors and enqueue on torch's current stream; only :func:`cell_table_device` synchronises, once, to learn the number
of cells.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np

from . import _native

CONNECTIVITIES = (4, 8)


class CellTable(NamedTuple):
    """Per-cell arrays, one row per cell, ordered by plane and then by id.  Device tensors, except the geometry columns
    (host float64 arrays, ``None`` without a geometry).  Indices are raw: a cell across the seam of ``wrap_rows`` is not
    unwrapped."""
    plane: object            # int32: the plane the cell lies in
    id: object               # int32: its label in that plane, from 1
    area: object             # int32: pixels
    bbox: object             # int32 [n, 4]: y_min, y_max, x_min, x_max
    sum_yx: object           # int64 [n, 2]: index sums; sum / area is the exact centroid in pixels
    vmax: object             # float32: the largest value
    argmax: object           # int32: its flat index y * w + x within the plane (the smallest among ties)
    vsum: object             # float64: sum of the values
    centroid_x: Optional[np.ndarray] = None
    centroid_y: Optional[np.ndarray] = None
    peak_x: Optional[np.ndarray] = None
    peak_y: Optional[np.ndarray] = None
    area_km2: Optional[np.ndarray] = None


def _is_tensor(a) -> bool:
    return type(a).__module__.startswith("torch")


def _check_planes(planes, what: str = "planes"):
    """Shape ``(n, h, w)`` of float32 ``[h, w]`` or ``[n, h, w]`` (tensor or ndarray), by dtype and rank only."""
    shape = tuple(int(n) for n in planes.shape)
    dtype = str(planes.dtype).replace("torch.", "")
    if dtype != "float32" or len(shape) not in (2, 3):
        raise ValueError(f"{what} must be float32 [h, w] or [n, h, w]; got {dtype} {list(shape)}")
    shape3 = (1,) + shape if len(shape) == 2 else shape
    if shape3[0] < 1:
        raise ValueError(f"{what}: no planes in shape {list(shape)}")
    if shape3[0] * shape3[1] * shape3[2] >= 2 ** 31:
        raise ValueError(f"{what}: {list(shape)} holds 2^31 pixels or more")
    return shape3


def _check_request(planes, threshold, upper, mask, connectivity, min_size=1):
    shape3 = _check_planes(planes)
    if connectivity not in CONNECTIVITIES or isinstance(connectivity, bool):
        raise ValueError(f"connectivity must be 4 or 8, not {connectivity!r}")
    lo, hi = float(np.float32(threshold)), float(np.float32(upper))
    if math.isnan(lo) or math.isnan(hi):
        raise ValueError(f"threshold and upper must not be NaN, got {threshold!r} and {upper!r}")
    if hi < lo:
        raise ValueError(f"upper {upper!r} lies below threshold {threshold!r}")
    if mask is not None and tuple(int(n) for n in mask.shape) != tuple(int(n) for n in planes.shape):
        raise ValueError(f"mask of shape {list(mask.shape)} for planes of shape {list(planes.shape)}")
    if isinstance(min_size, bool) or min_size != int(min_size) or not 1 <= min_size < 2 ** 31:
        raise ValueError(f"min_size must be an integer of at least 1, not {min_size!r}")
    return shape3, lo, hi


def _to_device(a, dev, dtype=None):
    torch = _native.torch_mod()
    t = a if _is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None and t.dtype != dtype:
        t = (t != 0 if dtype == torch.uint8 else t).to(dtype)        # a mask of another type: non-zero excludes
    return t.to(dev).contiguous()


def _device_of(a):
    if _is_tensor(a) and a.is_cuda:
        return a.device
    return _native.canonical_device(None)


def _label(lib, torch, src, mask_t, shape3, lo, hi, connectivity, wrap_rows):
    n, h, w = shape3
    dev = src.device
    labels = torch.empty(shape3, dtype=torch.int32, device=dev)
    cell_ptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
    need = int(lib.rg_components_workspace_bytes(n, h, w))
    if need < 0:
        _native.check(need, "rg_components_workspace_bytes")
    workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    _native.check(lib.rg_label_components_f32(_native.ptr(src), _native.ptr(mask_t), n, h, w, lo, hi, int(connectivity),
                                              1 if wrap_rows else 0, _native.ptr(labels), _native.ptr(cell_ptr),
                                              _native.ptr(workspace), need, _native.stream_ptr()), "rg_label_components_f32")
    return labels, cell_ptr


def label_components_device(planes, threshold, *, upper=float("inf"), mask=None, connectivity: int = 8,
                            wrap_rows: bool = False):
    """Label the connected regions of ``threshold <= planes <= upper`` (``rg_label_components_f32``).

    ``planes``: float32 ``[h, w]`` or ``[n, h, w]``, tensor or ndarray; ``mask``: optional, same shape, non-zero excludes.
    Returns ``(labels, cell_ptr)`` on the device: ``labels`` int32 of the planes' shape (0 background, cells from 1 per plane
    in raster order of their first pixel) and ``cell_ptr`` int32 ``[n + 1]``, the running count of cells -- cell ``k`` of
    plane ``p`` is row ``cell_ptr[p] + k - 1`` of a cell table.  ``wrap_rows``: row 0 and row ``h - 1`` of a plane are
    neighbours (a sweep's azimuth axis).  Planes never connect.  No host synchronisation."""
    shape3, lo, hi = _check_request(planes, threshold, upper, mask, connectivity)
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(planes)
    src = _to_device(planes, dev)
    mask_t = None if mask is None else _to_device(mask, dev, torch.uint8)
    with torch.cuda.device(dev):
        labels, cell_ptr = _label(lib, torch, src, mask_t, shape3, lo, hi, connectivity, wrap_rows)
    return labels.reshape(tuple(planes.shape)), cell_ptr


def _axes(geometry, h, w):
    shape, limits = tuple(geometry.grid_shape)[-2:], tuple(geometry.grid_limits)[-2:]
    if tuple(int(v) for v in shape) != (h, w):
        raise ValueError(f"geometry of planes {list(shape)} for planes of {[h, w]}")
    (y_lo, y_hi), (x_lo, x_hi) = ((float(a), float(b)) for a, b in limits)
    step_y = (y_hi - y_lo) / (h - 1) if h > 1 else 0.0
    step_x = (x_hi - x_lo) / (w - 1) if w > 1 else 0.0
    return y_lo, step_y, x_lo, step_x


def _stats(lib, torch, src, labels, cell_ptr, shape3, n_cells):
    n, h, w = shape3
    dev = src.device
    area = torch.empty(n_cells, dtype=torch.int32, device=dev)
    bbox = torch.empty((n_cells, 4), dtype=torch.int32, device=dev)
    sum_yx = torch.empty((n_cells, 2), dtype=torch.int64, device=dev)
    vmax = torch.empty(n_cells, dtype=torch.float32, device=dev)
    argmax = torch.empty(n_cells, dtype=torch.int32, device=dev)
    vsum = torch.empty(n_cells, dtype=torch.float64, device=dev)
    _native.check(lib.rg_component_stats_f32(_native.ptr(src), _native.ptr(labels), _native.ptr(cell_ptr), n, h, w, n_cells,
                                             _native.ptr(area), _native.ptr(bbox), _native.ptr(sum_yx), _native.ptr(vmax),
                                             _native.ptr(argmax), _native.ptr(vsum), _native.stream_ptr()),
                  "rg_component_stats_f32")
    return area, bbox, sum_yx, vmax, argmax, vsum


def cell_table_device(planes, labels, cell_ptr, geometry=None) -> CellTable:
    """The table of the cells of ``labels`` / ``cell_ptr`` (from :func:`label_components_device`) over the values of
    ``planes`` (``rg_component_stats_f32``).  Reads ``cell_ptr[-1]`` once -- the ONE host synchronisation of this module --
    then allocates the per-cell tensors and fills them.

    ``geometry``: anything with ``grid_shape`` / ``grid_limits`` whose last two axes are the planes' (a ``GridGeometry``);
    with it the table also carries, as host float64 arrays, ``centroid_x`` / ``centroid_y`` and ``peak_x`` / ``peak_y`` in
    metres -- ``lo + (sum / area) * step`` resp. ``lo + index * step`` on the float64 ``linspace`` axes of the grid -- and
    ``area_km2``."""
    shape3 = _check_planes(planes)
    if tuple(int(v) for v in labels.shape) != tuple(int(v) for v in planes.shape):
        raise ValueError(f"labels of shape {list(labels.shape)} for planes of shape {list(planes.shape)}")
    n, h, w = shape3
    axes = None if geometry is None else _axes(geometry, h, w)
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(labels)
    src = _to_device(planes, dev)
    labels = _to_device(labels, dev, torch.int32)
    cell_ptr = _to_device(cell_ptr, dev, torch.int32)
    if tuple(cell_ptr.shape) != (n + 1,):
        raise ValueError(f"cell_ptr of shape {list(cell_ptr.shape)} for {n} planes")
    n_cells = int(cell_ptr[-1].item())                         # the one synchronisation
    with torch.cuda.device(dev):
        area, bbox, sum_yx, vmax, argmax, vsum = _stats(lib, torch, src, labels, cell_ptr, shape3, n_cells)
        rows = torch.arange(n_cells, dtype=torch.int32, device=dev)
        plane = (torch.searchsorted(cell_ptr[1:].contiguous(), rows, right=True)).to(torch.int32)
        ids = rows - cell_ptr[plane.long()] + 1
    extra = {}
    if axes is not None:
        y_lo, step_y, x_lo, step_x = axes
        a = area.cpu().numpy().astype(np.float64)
        s = sum_yx.cpu().numpy().astype(np.float64)
        peak = argmax.cpu().numpy().astype(np.int64)
        extra = dict(centroid_x=x_lo + (s[:, 1] / a) * step_x, centroid_y=y_lo + (s[:, 0] / a) * step_y,
                     peak_x=x_lo + (peak % w).astype(np.float64) * step_x, peak_y=y_lo + (peak // w).astype(np.float64) * step_y,
                     area_km2=a * (step_x * step_y) / 1e6)
    return CellTable(plane, ids, area, bbox, sum_yx, vmax, argmax, vsum, **extra)


def despeckle_device(planes, threshold, min_size, *, upper=float("inf"), mask=None, connectivity: int = 8,
                     wrap_rows: bool = False, fill_value: float = float("nan"), return_mask: bool = False):
    """Planes with every echo region of fewer than ``min_size`` pixels set to ``fill_value``; all other pixels, background
    included, keep their bits (label -> areas -> ``rg_despeckle_select_f32``, no host synchronisation).

    Arguments as :func:`label_components_device`.  ``return_mask=True`` returns ``(out, removed)``, ``removed`` a uint8
    tensor of the planes' shape that is 1 where a pixel was removed: for a sweep ``[n_rays, n_gates]`` labelled with
    ``wrap_rows=True`` this is a gate mask for the gridders' ``masks`` arguments."""
    shape3, lo, hi = _check_request(planes, threshold, upper, mask, connectivity, min_size)
    n, h, w = shape3
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(planes)
    src = _to_device(planes, dev)
    mask_t = None if mask is None else _to_device(mask, dev, torch.uint8)
    with torch.cuda.device(dev):
        labels, cell_ptr = _label(lib, torch, src, mask_t, shape3, lo, hi, connectivity, wrap_rows)
        # a plane holds at most ceil(h / 2) * ceil(w / 2) cells under 8-connectivity, every other pixel under 4: the area
        # array is sized for that, so the cell count never has to come back to the host
        most = n * (((h * w + 1) // 2) if connectivity == 4 else ((h + 1) // 2) * ((w + 1) // 2))
        area = torch.empty(max(most, 1), dtype=torch.int32, device=dev)
        _native.check(lib.rg_component_stats_f32(_native.ptr(src), _native.ptr(labels), _native.ptr(cell_ptr), n, h, w, most,
                                                 _native.ptr(area), 0, 0, 0, 0, 0, _native.stream_ptr()),
                      "rg_component_stats_f32")
        out = torch.empty(tuple(planes.shape), dtype=torch.float32, device=dev)
        removed = torch.empty(tuple(planes.shape), dtype=torch.uint8, device=dev) if return_mask else None
        _native.check(lib.rg_despeckle_select_f32(_native.ptr(src), _native.ptr(labels), _native.ptr(cell_ptr), _native.ptr(area),
                                                  n, h, w, int(min_size), float(fill_value), _native.ptr(out),
                                                  _native.ptr(removed), _native.stream_ptr()), "rg_despeckle_select_f32")
    return (out, removed) if return_mask else out


def despeckle(planes, threshold, min_size, *, upper=float("inf"), mask=None, connectivity: int = 8, wrap_rows: bool = False,
              fill_value: float = float("nan"), return_mask: bool = False):
    """:func:`despeckle_device` for NumPy arrays: ndarray in, ndarray (or a pair of them) out."""
    got = despeckle_device(np.asarray(planes), threshold, min_size, upper=upper, mask=mask, connectivity=connectivity,
                           wrap_rows=wrap_rows, fill_value=fill_value, return_mask=return_mask)
    if return_mask:
        return got[0].cpu().numpy(), got[1].cpu().numpy()
    return got.cpu().numpy()


def identify_cells(plane, geometry, threshold, min_size: int = 1, connectivity: int = 8) -> dict:
    """The storm cells of one plane ``[h, w]``: connected regions of ``plane >= threshold`` with at least ``min_size`` pixels,
    as a dict of NumPy arrays ordered by id -- ``id``, ``area``, ``bbox``, ``sum_yx``, ``vmax``, ``argmax``, ``vsum`` and,
    with a ``geometry`` (may be ``None``), ``centroid_x``, ``centroid_y``, ``peak_x``, ``peak_y``, ``area_km2``.  Ids are the
    labelling's own: cells below ``min_size`` leave gaps."""
    plane = np.asarray(plane)
    if plane.ndim != 2:
        raise ValueError(f"plane must be float32 [h, w]; got {plane.dtype} {list(plane.shape)}")
    _check_request(plane, threshold, float("inf"), None, connectivity, min_size)
    labels, cell_ptr = label_components_device(plane, threshold, connectivity=connectivity)
    table = cell_table_device(plane, labels, cell_ptr, geometry)
    keep = table.area.cpu().numpy() >= int(min_size)
    out = {}
    for name, col in table._asdict().items():
        if col is None or name == "plane":
            continue
        out[name] = (col.cpu().numpy() if _is_tensor(col) else col)[keep]
    return out
