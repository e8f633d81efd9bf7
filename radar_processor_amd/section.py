"""A vertical cross-section along any path, gridded straight from the gates (csrc/rg_roi_section.hip).

The reference's ``radar_grid`` can cut a finished 3-D grid along one grid row or column (``plot_vertical_cross_section``,
``mpl_visualization.py:343-435``: ``grid[:, y_index, :]``).  Here a *section* is ``n_points`` sample columns
``(xs[i], ys[i])`` -- anywhere inside the grid's rectangle, at any spacing -- times the ``nz`` levels of a
:class:`RoiSearch`, and the value at level ``k``, point ``i`` is what the reference would put into a voxel lying exactly
there (``radar_grid/compute.py:46-91`` with ``radar_grid/interpolate.py:69-104``): the weighted mean of the gates within
that point's radius of influence, not a resampling of the lattice.

Two routes, as for the lattice: :func:`section_fields_device` grids without a CSR (one pass, nothing kept);
:func:`compute_section_geometry` keeps the section's CSR as an ordinary :class:`GridGeometry` of shape
``(nz, 1, n_points)`` for repeated volumes.  :func:`section_path` samples a polyline; :func:`vertical_section` is the
NumPy-in / NumPy-out convenience.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _native
from .geometry_builder import WEIGHTINGS, RoiSearch, csr_from_counts
from .grid_geometry import GridGeometry
from .gridding import _coerce_filters, _host_field, _to_host
from .roi_grid import pack_and_grid


def section_path(vertices, spacing: float) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Sample the polyline through ``vertices`` (``[(x, y), ...]``, metres) every ``spacing`` metres of path length:
    ``s_j = j * spacing`` for ``j = 0 .. floor(L / spacing)``, ``L`` the polyline's length.  The position is interpolated
    linearly inside its segment in float64 and rounded to float32.  Returns ``(xs float32, ys float32, s float64)``; the
    last vertex is a sample only where ``L`` is a multiple of ``spacing``."""
    v = np.asarray(vertices, dtype=np.float64)
    if v.ndim != 2 or v.shape[1] != 2 or v.shape[0] < 2:
        raise ValueError("vertices must be at least two (x, y) pairs")
    spacing = float(spacing)
    if not np.all(np.isfinite(v)) or not math.isfinite(spacing):
        raise ValueError("vertices and spacing must be finite")
    if not spacing > 0.0:
        raise ValueError(f"spacing must be positive, not {spacing}")
    seg = np.hypot(np.diff(v[:, 0]), np.diff(v[:, 1]))
    if np.any(seg == 0.0):
        raise ValueError(f"segment {int(np.argmin(seg))} of the path has zero length")
    cum = np.concatenate([[0.0], np.cumsum(seg)])
    s = np.arange(int(math.floor(cum[-1] / spacing)) + 1, dtype=np.float64) * spacing
    k = np.clip(np.searchsorted(cum, s, side="right") - 1, 0, len(seg) - 1)      # the segment a sample lies in
    t = (s - cum[k]) / seg[k]
    xs = v[k, 0] + t * (v[k + 1, 0] - v[k, 0])
    ys = v[k, 1] + t * (v[k + 1, 1] - v[k, 1])
    return xs.astype(np.float32), ys.astype(np.float32), s


def _host(a):
    """A tensor (any device) -> NumPy; anything else as it is."""
    return a.detach().cpu().numpy() if hasattr(a, "detach") else a


def _length(a) -> int:
    """Element count of a NumPy array, torch tensor or sequence -- without touching a device."""
    if hasattr(a, "numel"):
        return int(a.numel())
    if hasattr(a, "size") and not callable(a.size):
        return int(a.size)
    return len(a)


def _upload(values: np.ndarray, mask: np.ndarray, dev):
    """A host field (``gridding._host_field``) on ``dev``: ``(values, mask)`` tensors, the mask only where it excludes a gate."""
    torch = _native.torch_mod()
    return torch.from_numpy(values).to(dev), torch.from_numpy(mask).to(dev) if mask.any() else None


def _grid_rectangle(grid_shape, grid_limits, window=None) -> Tuple[float, float, float, float]:
    """``(x_min, x_max, y_min, y_max)`` of the columns ``window = (iy0, iy1, ix0, ix1)`` (default: all) of a grid: the ends
    of its float32 coordinate tables there.  Host arithmetic: the tables are NumPy's float32 ``linspace``
    (``compute.py:185-186``), recomputed here rather than read back."""
    _, ny, nx = grid_shape
    iy0, iy1, ix0, ix1 = (0, ny, 0, nx) if window is None else window
    yc = np.linspace(grid_limits[1][0], grid_limits[1][1], ny, dtype="float32")[iy0:iy1]
    xc = np.linspace(grid_limits[2][0], grid_limits[2][1], nx, dtype="float32")[ix0:ix1]
    return float(xc.min()), float(xc.max()), float(yc.min()), float(yc.max())


def section_rectangle(search) -> Tuple[float, float, float, float]:
    """``(x_min, x_max, y_min, y_max)`` of the sample points a search structure serves: the xy rectangle of its
    ``grid_limits`` -- the ends of its float32 coordinate tables -- and for a windowed search the window's coordinate
    range.  The cell lattice and the padding by the largest radius of influence are proven only there.  Host arithmetic:
    the tables are NumPy's float32 ``linspace`` (``compute.py:185-186``), recomputed here rather than read back."""
    return _grid_rectangle(search.full_shape, search.grid_limits, search.window)


def _refuse_closest(weighting: str, what: str = "a section") -> None:
    """The weightings of a section (of ``what``): no closest-gate mode; raises ValueError, touches no device."""
    if weighting == "closest":
        raise ValueError(f"weighting 'closest' is a single-radar lattice mode; {what} takes barnes2, cressman or nearest")
    if weighting not in WEIGHTINGS:
        raise ValueError(f"Unknown weighting function: {weighting}")


def _check_points_in(rectangle, xs, ys):
    """The points as contiguous float32 host arrays, refused (``ValueError``) unless they are finite, one-dimensional, of
    equal length, at least one, and inside ``rectangle = (x0, x1, y0, y1)`` (its rim included).  Touches no device."""
    xs = np.ascontiguousarray(_host(xs), dtype=np.float32)
    ys = np.ascontiguousarray(_host(ys), dtype=np.float32)
    if xs.ndim != 1 or ys.ndim != 1 or xs.shape != ys.shape:
        raise ValueError(f"xs and ys must be one-dimensional and of equal length, not {xs.shape} and {ys.shape}")
    if xs.size == 0:
        raise ValueError("a section needs at least one point (n_points == 0)")
    if not (np.all(np.isfinite(xs)) and np.all(np.isfinite(ys))):
        raise ValueError("xs and ys must be finite (NaN or infinite coordinate)")
    x0, x1, y0, y1 = rectangle
    bad = (xs < x0) | (xs > x1) | (ys < y0) | (ys > y1)
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError(f"point {i} = ({xs[i]}, {ys[i]}) lies outside the rectangle x [{x0}, {x1}], y [{y0}, {y1}] the "
                         f"search was built for ({int(bad.sum())} of {xs.size} points do)")
    return xs, ys


def _check_points(search, xs, ys, weighting: str):
    """The weighting and the points of a section on ``search``, refused before anything touches the device."""
    _refuse_closest(weighting)
    return _check_points_in(section_rectangle(search), xs, ys)


def _cumulative_distance(xs: np.ndarray, ys: np.ndarray) -> float:
    x, y = xs.astype(np.float64), ys.astype(np.float64)
    return float(np.hypot(np.diff(x), np.diff(y)).sum())


def section_fields_device(search: RoiSearch, xs, ys, fields: Sequence, masks: Optional[Sequence] = None, shared_mask=None,
                          weighting: str = "barnes2", fill_value: float = np.nan, out=None):
    """Grid device-resident fields at the columns ``(xs[i], ys[i])`` straight from the gates, without a CSR.  ``xs`` /
    ``ys``: float32 metres in the radar frame (the frame of the gate coordinates), inside the search's rectangle
    (:func:`section_rectangle`); they need not be equally spaced, sorted or distinct -- only the speed depends on
    consecutive points being close.  ``fields`` / ``masks`` / ``shared_mask`` / ``fill_value`` / ``out`` as
    :func:`roi_grid_fields_device`.  Returns ``[F, nz, n_points]`` float32."""
    xs, ys = _check_points(search, xs, ys, weighting)
    if len(fields) == 0:
        raise ValueError("no fields to grid")
    fill = float(np.float32(fill_value))
    points = []       # the points on the device: copied once, by the first launch -- after everything has been validated

    def launch(packed, nf, stride, out_view, stream):
        if not points:
            torch = _native.torch_mod()
            points.extend((torch.from_numpy(xs).to(search.dev), torch.from_numpy(ys).to(search.dev)))
        _native.check(_native.load_library().rg_roi_section_f32(
            *_section_args(search, *points), _native.WEIGHTINGS[weighting], _native.ptr(packed), nf, stride, fill,
            _native.ptr(out_view), stream), "rg_roi_section_f32")
    return pack_and_grid(search.dev, search.n_gates, fields, masks, shared_mask, out,
                         (search.grid_shape[0], int(xs.size)), launch)


def _section_args(search: RoiSearch, xs_t, ys_t):
    """The ten leading arguments of the section entry points: the search structure, the points (device tensors the caller
    keeps alive), the levels, the ROI."""
    return (_native.ptr(search.sorted_gates), _native.ptr(search.cell_start), search.cells, _native.ptr(xs_t),
            _native.ptr(ys_t), _native.ptr(search.zc), search.grid_shape[0], int(xs_t.numel()), search.min_radius,
            search.beam_factor)


class _PathRows:
    """The count and fill pair of one path search (``rg_section_count_f32`` / ``rg_section_fill_f32``): the rows
    ``k * n_points + i`` of the points ``(xs[i], ys[i])`` -- float32 host arrays in the frame of ``search`` -- times its
    levels.  Keeps the points alive on the device; call it under ``torch.cuda.device(search.dev)``."""

    def __init__(self, search: RoiSearch, xs: np.ndarray, ys: np.ndarray):
        torch = _native.torch_mod()
        self.points = torch.from_numpy(xs).to(search.dev), torch.from_numpy(ys).to(search.dev)
        self.head = _section_args(search, *self.points)
        self.n_rows = search.grid_shape[0] * int(xs.size)
        self.dev = search.dev

    def count(self):
        """int32 ``[n_rows + 1]``: every row's number of neighbours and a trailing zero."""
        torch = _native.torch_mod()
        counts = torch.zeros(self.n_rows + 1, dtype=torch.int32, device=self.dev)
        _native.check(_native.load_library().rg_section_count_f32(*self.head, _native.ptr(counts), _native.stream_ptr()),
                      "rg_section_count_f32")
        return counts

    def fill(self, weighting: str, indptr, gate_idx, weights) -> None:
        """Row v's pairs go to positions ``indptr[v] ...`` of the two arrays."""
        _native.check(_native.load_library().rg_section_fill_f32(
            *self.head, _native.WEIGHTINGS[weighting], _native.ptr(indptr), _native.ptr(gate_idx), _native.ptr(weights),
            _native.stream_ptr()), "rg_section_fill_f32")


def compute_section_geometry(search: RoiSearch, xs, ys, weighting: str = "barnes2") -> GridGeometry:
    """The section's CSR as an ordinary geometry: ``grid_shape (nz, 1, n_points)``, row ``k * n_points + i`` holding the
    gates within the radius of influence of ``(xs[i], ys[i], z_k)`` and their weights (float64-exact, rounded to float32,
    as ``compute_grid_geometry`` writes them).  It goes through ``apply_geometry`` / ``apply_geometry_multi`` /
    ``grid_fields_device`` / ``save_geometry`` like any geometry -- the route for repeated volumes.  ``grid_limits`` are
    ``(z_limits, (0.0, 0.0), (0.0, s_last))`` with ``s_last`` the cumulative point-to-point distance; the points
    themselves are kept as ``.section_x`` / ``.section_y`` (``save_geometry`` writes the reference's nine keys only)."""
    xs, ys = _check_points(search, xs, ys, weighting)
    nz, n_points = search.grid_shape[0], int(xs.size)
    with _native.torch_mod().cuda.device(search.dev):
        rows = _PathRows(search, xs, ys)
        csr = csr_from_counts(rows.count(), rows.n_rows, lambda *csr_arrays: rows.fill(weighting, *csr_arrays))
    z_limits = tuple(float(v) for v in search.grid_limits[0])
    geom = GridGeometry.from_device((nz, 1, n_points), (z_limits, (0.0, 0.0), (0.0, _cumulative_distance(xs, ys))),
                                    csr, search.toa)
    geom.section_x, geom.section_y = xs, ys
    return geom


def vertical_section(gate_x, gate_y, gate_z, field_data, vertices, spacing, z_limits, nz, additional_filters=None,
                     radar_altitude=0.0, min_radius=250.0, beam_factor=0.01746, weighting="barnes2", toa=17000.0,
                     fill_value=np.nan):
    """One masked field on the vertical section along the polyline ``vertices`` sampled every ``spacing`` metres
    (:func:`section_path`), ``nz`` levels over ``z_limits``; the gridding arguments as ``compute_grid_geometry`` and
    ``apply_geometry``.  Returns ``(section float32 [nz, n_points], s float64 [n_points])``.

    The search structure is built for the bounding box of the float32 sample points themselves, so every sample lies
    inside its rectangle by construction (a path along an axis gives a rectangle of zero width, which is legal)."""
    xs, ys, s = section_path(vertices, spacing)
    nz = int(nz)
    if nz < 1:
        raise ValueError(f"nz must be at least 1, not {nz}")
    _refuse_closest(weighting)
    values, mask = _host_field(field_data, _coerce_filters(additional_filters))
    limits = (tuple(float(v) for v in z_limits), (float(ys.min()), float(ys.max())), (float(xs.min()), float(xs.max())))
    search = RoiSearch(gate_x, gate_y, gate_z, (nz, 2, 2), limits, radar_altitude=radar_altitude, min_radius=min_radius,
                       beam_factor=beam_factor, toa=toa)
    if values.size != search.n_gates:
        raise ValueError(f"field_data has {values.size} values for {search.n_gates} gates")
    f_t, m_t = _upload(values, mask, search.dev)
    out = section_fields_device(search, xs, ys, [f_t], [m_t], weighting=weighting, fill_value=fill_value)
    return _to_host(out[0]), s
