"""Restatement of the connected-component contract of include/radargrid_hip.h ("Connected echo regions") in plain Python:
a raster-order flood fill with connectivity, row wrap and mask, the per-cell table with exact integer sums and ``math.fsum``,
and despeckling.  Slow and obvious on purpose; the GPU tests compare the kernels against it, the CPU tests compare it against
``scipy.ndimage.label`` and hand-written answers."""
import math
import struct
from collections import deque

import numpy as np


def foreground(planes, lo, hi=np.inf, mask=None):
    """``v >= lo && v <= hi`` in float32 and the mask zero; NaN fails both comparisons."""
    planes = np.asarray(planes, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        fg = (planes >= np.float32(lo)) & (planes <= np.float32(hi))
    if mask is not None:
        fg &= np.asarray(mask) == 0
    return fg


def neighbours(y, x, h, w, connectivity, wrap_rows):
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    if connectivity == 8:
        steps += [(-1, -1), (-1, 1), (1, -1), (1, 1)]
    for dy, dx in steps:
        yy, xx = y + dy, x + dx
        if wrap_rows:
            yy %= h
        if 0 <= yy < h and 0 <= xx < w:
            yield yy, xx


def label_plane(fg, connectivity=8, wrap_rows=False):
    """Labels of one boolean plane: cells numbered from 1 in raster order of their first pixel."""
    fg = np.asarray(fg, dtype=bool)
    h, w = fg.shape
    labels = np.zeros((h, w), dtype=np.int32)
    count = 0
    for y0 in range(h):
        for x0 in range(w):
            if not fg[y0, x0] or labels[y0, x0]:
                continue
            count += 1
            labels[y0, x0] = count
            todo = deque([(y0, x0)])
            while todo:
                y, x = todo.popleft()
                for yy, xx in neighbours(y, x, h, w, connectivity, wrap_rows):
                    if fg[yy, xx] and not labels[yy, xx]:
                        labels[yy, xx] = count
                        todo.append((yy, xx))
    return labels, count


def label(planes, lo, hi=np.inf, mask=None, connectivity=8, wrap_rows=False):
    """``(labels int32 [n, h, w], cell_ptr int32 [n + 1])`` of float32 planes ``[n, h, w]``."""
    planes = np.asarray(planes, dtype=np.float32)
    assert planes.ndim == 3
    fg = foreground(planes, lo, hi, mask)
    labels = np.zeros(planes.shape, dtype=np.int32)
    cell_ptr = np.zeros(planes.shape[0] + 1, dtype=np.int32)
    for p in range(planes.shape[0]):
        labels[p], n = label_plane(fg[p], connectivity, wrap_rows)
        cell_ptr[p + 1] = cell_ptr[p] + n
    return labels, cell_ptr


def total_order_key(v):
    """Integer that orders non-NaN float32 values by the IEEE total order (-0 below +0)."""
    bits = struct.unpack("<I", struct.pack("<f", float(v)))[0]
    return bits ^ 0xFFFFFFFF if bits >> 31 else bits ^ 0x80000000


def stats(planes, labels, cell_ptr):
    """The cell table as a dict of arrays with ``cell_ptr[-1]`` rows.  Indices are raw (no unwrapping).  ``vsum`` is the
    correctly rounded sum (``math.fsum``), ``abs_sum`` the float64 sum of magnitudes the vsum bound is stated in."""
    planes = np.asarray(planes, dtype=np.float32)
    n, h, w = planes.shape
    cells = int(cell_ptr[-1])
    out = dict(plane=np.zeros(cells, np.int32), id=np.zeros(cells, np.int32), area=np.zeros(cells, np.int32),
               bbox=np.zeros((cells, 4), np.int32), sum_yx=np.zeros((cells, 2), np.int64), vmax=np.zeros(cells, np.float32),
               argmax=np.zeros(cells, np.int32), vsum=np.zeros(cells, np.float64), abs_sum=np.zeros(cells, np.float64))
    for p in range(n):
        flat = np.asarray(labels[p]).ravel()
        pixels = np.nonzero(flat)[0]
        pixels = pixels[np.argsort(flat[pixels], kind="stable")]          # by cell, raster order within a cell
        ends = np.cumsum(np.bincount(flat[pixels], minlength=int(cell_ptr[p + 1] - cell_ptr[p]) + 1))
        for k in range(1, int(cell_ptr[p + 1] - cell_ptr[p]) + 1):
            row = int(cell_ptr[p]) + k - 1
            ys, xs = np.divmod(pixels[ends[k - 1]:ends[k]], w)
            vals = planes[p, ys, xs]
            out["plane"][row], out["id"][row], out["area"][row] = p, k, len(ys)
            out["bbox"][row] = [ys.min(), ys.max(), xs.min(), xs.max()]
            out["sum_yx"][row] = [int(ys.astype(np.int64).sum()), int(xs.astype(np.int64).sum())]
            best, best_key = -1, -1
            for j, v in enumerate(vals):
                if not np.isnan(v) and total_order_key(v) > best_key:      # strict: ties keep the smallest index
                    best, best_key = j, total_order_key(v)
            out["vmax"][row] = vals[best] if best >= 0 else np.float32(np.nan)
            out["argmax"][row] = ys[best] * w + xs[best] if best >= 0 else -1
            out["vsum"][row] = math.fsum(float(v) for v in vals)
            out["abs_sum"][row] = math.fsum(abs(float(v)) for v in vals)
    return out


def despeckle_labelled(planes, labels, cell_ptr, min_size, fill=np.nan):
    """``(out, removed uint8)`` from a labelling: cells smaller than ``min_size`` pixels set to ``fill``, every other pixel
    bit for bit."""
    planes = np.asarray(planes, dtype=np.float32)
    out = planes.copy()
    removed = np.zeros(planes.shape, dtype=np.uint8)
    for p in range(planes.shape[0]):
        areas = np.bincount(labels[p].ravel(), minlength=int(cell_ptr[p + 1] - cell_ptr[p]) + 1)
        small = (labels[p] > 0) & (areas[labels[p]] < min_size)
        out[p][small] = np.float32(fill)
        removed[p][small] = 1
    return out, removed


def despeckle(planes, lo, min_size, hi=np.inf, mask=None, connectivity=8, wrap_rows=False, fill=np.nan):
    planes = np.asarray(planes, dtype=np.float32)
    return despeckle_labelled(planes, *label(planes, lo, hi, mask, connectivity, wrap_rows), min_size, fill)


def partition(labels):
    """The set of cells as frozensets of flat indices: what two labellings share when only the numbering differs."""
    flat = np.asarray(labels).ravel()
    cells = {}
    for i in np.nonzero(flat)[0]:
        cells.setdefault(int(flat[i]), []).append(int(i))
    return {frozenset(v) for v in cells.values()}


def centroids(table, grid_shape, grid_limits):
    """The host float64 formula of ``cell_table_device``: ``lo + (sum / area) * step`` on the float64 linspace axes."""
    (ny, nx), (ylim, xlim) = tuple(grid_shape)[-2:], tuple(grid_limits)[-2:]
    step_y = (float(ylim[1]) - float(ylim[0])) / (ny - 1) if ny > 1 else 0.0
    step_x = (float(xlim[1]) - float(xlim[0])) / (nx - 1) if nx > 1 else 0.0
    area = table["area"].astype(np.float64)
    sums = table["sum_yx"].astype(np.float64)
    peak = table["argmax"].astype(np.int64)
    return dict(centroid_y=float(ylim[0]) + (sums[:, 0] / area) * step_y, centroid_x=float(xlim[0]) + (sums[:, 1] / area) * step_x,
                peak_y=float(ylim[0]) + (peak // nx).astype(np.float64) * step_y,
                peak_x=float(xlim[0]) + (peak % nx).astype(np.float64) * step_x,
                area_km2=area * (step_x * step_y) / 1e6)
