"""Several radars on one shared grid (mosaic).

Each radar gives float32 gate coordinates relative to its antenna (what ``get_gate_coordinates`` returns) and its
``origin = (oz, oy, ox)``: the antenna position in the grid frame, in metres, in the axis order of ``grid_limits``.  Gates
are translated into the grid frame, not rotated or re-projected.

Radar r's contribution to voxel v is row v of ``compute_grid_geometry(gx_r, gy_r, gz_r, grid_shape,
mosaic_limits(grid_limits, o_r), ..., radar_altitude=0.0, toa=toa - oz_r)`` -- the reference's neighbour set and weights
(``radar_grid/compute.py:46-91``) in that radar's frame.  The mosaic value of a voxel is the masked weighted mean
(``radar_grid/interpolate.py:69-104``) over the union of every radar's neighbours::

    sum_r sum_{live j} w_j * v_j / sum_r sum_{live j} w_j          (fill_value where the weight sum is not > 0)

Radar r's gate g is gate ``gate_offsets[r] + g`` of the mosaic (radars concatenated in the order given), and row v of a
mosaic geometry is radar 0's row v, then radar 1's, and so on.  With one radar at origin (0, 0, 0) the mosaic IS
``compute_grid_geometry``.

Two routes:

* :func:`compute_mosaic_geometry` builds one reference-format CSR over the concatenated gates (the builder's count and
  fill kernels, each radar over its reach window) and :func:`apply_mosaic` / :func:`mosaic_fields_device` grid through it
  like any geometry -- for repeated volumes;
* :class:`MosaicSearch` keeps one search structure per radar and :func:`mosaic_fields_device` grids straight from the gates
  (``rg_roi_grid_mosaic_f32``) -- no CSR, any subset of the radars per call.

A vertical section through a mosaic (``csrc/rg_roi_section.hip``: ``rg_roi_section_mosaic_f32``) has the same two routes:
:func:`mosaic_section_fields_device` on a :class:`MosaicSearch` -- of a lattice, or of the path itself
(:meth:`MosaicSearch.for_path`) -- and :func:`compute_mosaic_section_geometry`; :func:`mosaic_vertical_section` is the
NumPy-in / NumPy-out convenience.  The points are given in the grid frame and seen from every radar's own frame
(:func:`mosaic_section_points`).
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from .geometry_builder import _INT32_MAX, WEIGHTINGS, RoiSearch, csr_from_counts
from .grid_geometry import GridGeometry
from .gridding import _coerce_filters, _host_field, _stride_for, _to_host, grid_fields_device
from .plane_products import ProductPlan, grid_products_device
from .roi_grid import pack_and_grid
from .section import _check_points, _cumulative_distance, section_path, section_rectangle

_GATHER_BYTES = 2 ** 32        # buffer-resource range of the packed-field gather in rg_csr_apply_f32
MOSAIC_COMBINES = tuple(_native.COMBINES)      # "mean", "max", "nearest_radar": the combine rules of the CSR-free route
NO_RADAR = _native.RG_NO_RADAR                 # in a ``radar`` map: no radar has a value there (the grid holds the fill)


def mosaic_limits(grid_limits, origin) -> Tuple[Tuple[float, float], ...]:
    """The shared grid's limits in the frame of a radar at ``origin = (oz, oy, ox)`` (Python floats)."""
    return tuple((float(lo) - float(o), float(hi) - float(o)) for (lo, hi), o in zip(grid_limits, origin))


def _length(a) -> int:
    """Element count of a NumPy array, torch tensor or sequence -- without touching a device."""
    if hasattr(a, "numel"):
        return int(a.numel())
    if hasattr(a, "size") and not callable(a.size):
        return int(a.size)
    return len(a)


def _host(a):
    """A tensor (any device) -> NumPy; anything else as it is."""
    return a.detach().cpu().numpy() if hasattr(a, "detach") else a


def _check_radars(radars, max_radars: Optional[int] = None):
    """``[(gate_x, gate_y, gate_z, origin), ...]`` -> (gate counts, origins float64 [R, 3]); raises ValueError."""
    radars = list(radars)
    if not radars:
        raise ValueError("a mosaic needs at least one radar")
    if max_radars is not None and len(radars) > max_radars:
        raise ValueError(f"{len(radars)} radars: one CSR-free mosaic launch takes at most {max_radars} "
                         "(RG_MAX_RADARS); build a mosaic geometry instead")
    counts, origins = [], []
    for r, radar in enumerate(radars):
        if len(radar) != 4:
            raise ValueError(f"radar {r}: expected (gate_x, gate_y, gate_z, origin)")
        gx, gy, gz, origin = radar
        o = np.asarray(origin, dtype=np.float64)
        if o.shape != (3,) or not np.all(np.isfinite(o)):
            raise ValueError(f"radar {r}: origin must be three finite numbers (oz, oy, ox), got {origin!r}")
        n = _length(gx)
        if not (_length(gy) == _length(gz) == n):
            raise ValueError(f"radar {r}: gate_x, gate_y and gate_z differ in length")
        counts.append(n)
        origins.append(o)
    if sum(counts) > _INT32_MAX:
        raise ValueError(f"{sum(counts)} gates in all: the mosaic numbers gates with int32 (at most 2^31 - 1)")
    return counts, np.stack(origins)


def _offsets(counts: Sequence[int]) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.int64))]).astype(np.int64)


def _reach_box(gate_x, gate_y, gate_z, origin, min_radius: float, beam_factor: float, toa: float):
    """``(x_lo, x_hi, y_lo, y_hi)`` of the valid gates ``+- R_g`` in the radar's frame (:func:`reach_window` says what
    ``R_g`` is), or ``None`` when no gate is valid.  ``beam_factor`` must lie in ``[0, 1)``.  Host code, float64."""
    gx = np.asarray(_host(gate_x), dtype=np.float32).ravel().astype(np.float64)
    gy = np.asarray(_host(gate_y), dtype=np.float32).ravel().astype(np.float64)
    gz32 = np.asarray(_host(gate_z), dtype=np.float32).ravel()
    valid = (gz32 <= np.float32(float(toa) - float(origin[0]))) & np.isfinite(gx) & np.isfinite(gy)
    if not valid.any():
        return None
    gx, gy, gz = gx[valid], gy[valid], gz32[valid].astype(np.float64)
    bf = float(beam_factor)
    reach = np.maximum(float(min_radius), bf * np.sqrt(gx * gx + gy * gy + gz * gz) / (1.0 - bf))
    reach = reach * (1.0 + 1e-9) + 1e-6         # the bound is exact arithmetic; the float64 test rounds
    return (float(np.min(gx - reach)), float(np.max(gx + reach)), float(np.min(gy - reach)), float(np.max(gy + reach)))


def path_reach(gate_x, gate_y, gate_z, origin, rectangle, min_radius: float = 250.0, beam_factor: float = 0.01746,
               toa: float = 17000.0) -> bool:
    """Whether a radar at ``origin = (oz, oy, ox)`` can have a neighbour of any point inside ``rectangle =
    (x_min, x_max, y_min, y_max)`` (grid frame, metres): whether the xy box of its valid gates ``+- R_g`` meets the
    rectangle, with :func:`reach_window`'s ``R_g`` and inflation.  ``False`` is a proof (no gate is within its reach of
    any point of the rectangle, at any height); ``True`` is not one.  ``beam_factor`` outside ``[0, 1)``: ``True``.  Host
    code, float64; touches no device."""
    x0, x1, y0, y1 = (float(v) for v in rectangle)
    o = np.asarray(origin, dtype=np.float64)
    if o.shape != (3,) or not np.all(np.isfinite(o)):
        raise ValueError(f"origin must be three finite numbers (oz, oy, ox), got {origin!r}")
    if not (x0 <= x1 and y0 <= y1):
        raise ValueError(f"rectangle must be (x_min, x_max, y_min, y_max), got {rectangle!r}")
    if not (0.0 <= float(beam_factor) < 1.0):
        return True
    box = _reach_box(gate_x, gate_y, gate_z, o, min_radius, beam_factor, toa)
    if box is None:
        return False
    oy, ox = float(o[1]), float(o[2])
    return bool(box[0] <= x1 - ox and box[1] >= x0 - ox and box[2] <= y1 - oy and box[3] >= y0 - oy)


def reach_window(gate_x, gate_y, gate_z, grid_shape, grid_limits, origin, min_radius: float = 250.0,
                 beam_factor: float = 0.01746, toa: float = 17000.0) -> Tuple[int, int, int, int]:
    """The columns ``(iy0, iy1, ix0, ix1)`` (half-open) of the shared grid a radar can reach.

    A valid gate (``gz <= toa - oz``) is a neighbour only of voxels within ``R_g = max(min_radius, bf * |g| / (1 - bf))`` of
    it (the bound ``rg_geom_bin_levels_count`` uses: ``r_v = max(min_radius, |v| * bf)`` and ``|v| <= |g| + r_v``).  The
    window holds the voxels whose coordinates -- the radar's own float32 tables of the shifted limits -- fall inside the
    xy box of ``gate +- R_g``, widened by one voxel on each side and clipped to the grid.  ``iy0 == iy1``: the radar reaches
    nothing.  ``beam_factor`` outside ``[0, 1)``: the whole grid.  Host code, float64; gate coordinates may be NumPy arrays or
    tensors on any device (they are copied to the host)."""
    nz, ny, nx = (int(s) for s in grid_shape)
    if not (0.0 <= float(beam_factor) < 1.0):
        return (0, ny, 0, nx)
    lim = mosaic_limits(grid_limits, origin)
    box = _reach_box(gate_x, gate_y, gate_z, origin, min_radius, beam_factor, toa)
    if box is None:
        return (0, 0, 0, 0)
    yc = np.linspace(lim[1][0], lim[1][1], ny, dtype="float32").astype(np.float64)
    xc = np.linspace(lim[2][0], lim[2][1], nx, dtype="float32").astype(np.float64)

    def span(c, lo, hi):
        idx = np.nonzero((c >= lo) & (c <= hi))[0]
        if idx.size == 0:
            return 0, 0
        return max(int(idx.min()) - 1, 0), min(int(idx.max()) + 2, len(c))

    iy0, iy1 = span(yc, box[2], box[3])
    ix0, ix1 = span(xc, box[0], box[1])
    if iy0 == iy1 or ix0 == ix1:
        return (0, 0, 0, 0)
    return (iy0, iy1, ix0, ix1)


def _window_empty(w) -> bool:
    return w[0] >= w[1] or w[2] >= w[3]


# ------------------------------------------------------------------------------------------------------------------------
# geometry route
# ------------------------------------------------------------------------------------------------------------------------
def compute_mosaic_geometry(radars, grid_shape, grid_limits, temp_dir: str, min_radius: float = 250.0,
                            beam_factor: float = 0.01746, weighting: str = "barnes2", toa: float = 17000.0,
                            n_workers: Optional[int] = None) -> GridGeometry:
    """One reference-format geometry of several radars on one grid: row v is radar 0's row v of
    ``compute_grid_geometry(..., mosaic_limits(grid_limits, o_r), radar_altitude=0.0, toa=toa - oz_r)``, then radar 1's, ...,
    with radar r's gate g numbered ``gate_offsets[r] + g``.

    ``radars``: a sequence of ``(gate_x, gate_y, gate_z, origin)``.  The result carries the shared ``grid_limits`` and
    ``toa`` and, besides the reference's arrays, ``.gate_offsets`` (int64 ``[R + 1]``) and ``.origins`` (float64 ``[R, 3]``).
    ``save_geometry`` writes the usual nine keys: a reloaded mosaic is a plain geometry over the concatenated gates (the
    two mosaic attributes are not kept).  Geometries of 50 M pairs and more get the compact / packed device copy on their
    first gridding pass like any other (``gridding._use_compact``); only the CSR layout is built here.  ``temp_dir`` and
    ``n_workers`` as in ``compute_grid_geometry``."""
    if not os.path.isdir(temp_dir):
        raise ValueError(f"temp_dir does not exist: {temp_dir}")
    if weighting not in WEIGHTINGS:
        raise ValueError(f"Unknown weighting function: {weighting}")
    radars = list(radars)
    counts, origins = _check_radars(radars)
    torch = _native.torch_mod()
    _native.load_library()
    dev = _native.device()
    nz, ny, nx = (int(s) for s in grid_shape)
    n_vox = nz * ny * nx
    offsets = _offsets(counts)
    # per radar: its search over its reach window (None: reaches nothing)
    parts = []
    for r, (gx, gy, gz, origin) in enumerate(radars):
        w = reach_window(gx, gy, gz, (nz, ny, nx), grid_limits, origins[r], min_radius, beam_factor, toa)
        if _window_empty(w):
            parts.append(None)
            continue
        search = RoiSearch(gx, gy, gz, (nz, ny, nx), mosaic_limits(grid_limits, origins[r]), radar_altitude=0.0,
                           min_radius=min_radius, beam_factor=beam_factor, toa=float(toa) - float(origins[r][0]),
                           device=dev, window=w)
        parts.append(search)
    with torch.cuda.device(dev):
        total = torch.zeros(n_vox + 1, dtype=torch.int32, device=dev)
        grid_counts = total[:n_vox].view(nz, ny, nx)
        win_counts = []
        for search in parts:
            if search is None:
                win_counts.append(None)
                continue
            iy0, iy1, ix0, ix1 = search.window
            win_counts.append(search.count_rows()[:-1].view(search.grid_shape))
            grid_counts[:, iy0:iy1, ix0:ix1] += win_counts[-1]

        def fill(indptr, gate_idx, weights):
            # running cursor: indptr plus the counts of the radars already filled.  The fill kernel reads only cursor[v] as
            # the row base and writes at absolute positions, so every radar fills its segment of each row of its window.
            cursor = indptr[:n_vox].view(nz, ny, nx).clone()
            for r, search in enumerate(parts):
                if search is None:
                    continue
                iy0, iy1, ix0, ix1 = search.window
                cur_w = cursor[:, iy0:iy1, ix0:ix1].contiguous()
                # the radar's gate numbers carry its offset: shift the index column of this build's copy of its sorted gates
                search.sorted_gates.view(torch.int32).view(-1, 4)[:, 3] += int(offsets[r])
                search.fill_rows(weighting, _native.ptr(cur_w), _native.ptr(gate_idx), _native.ptr(weights))
                cursor[:, iy0:iy1, ix0:ix1] += win_counts[r]
        csr = csr_from_counts(total, n_vox, fill)
        del parts
    geom = GridGeometry.from_device((nz, ny, nx), grid_limits, csr, toa)
    geom.gate_offsets = offsets
    geom.origins = origins
    return geom


def _mosaic_layout(geometry) -> np.ndarray:
    offsets = getattr(geometry, "gate_offsets", None)
    if offsets is None:
        raise ValueError("not a mosaic: the geometry has no gate_offsets (built by compute_mosaic_geometry)")
    return np.asarray(offsets, dtype=np.int64)


def _host_concat(offsets, fields, filters, what: str):
    """Per-radar masked fields (+ per-radar GateFilter lists) -> concatenated float32 values and uint8 exclusion mask."""
    n_radars = len(offsets) - 1
    if len(fields) != n_radars:
        raise ValueError(f"{what}: expected one field per radar ({n_radars}), got {len(fields)}")
    if filters is None:
        filters = [None] * n_radars
    if len(filters) != n_radars:
        raise ValueError(f"{what}: expected one filter list per radar ({n_radars}), got {len(filters)}")
    values, masks = [], []
    for r in range(n_radars):
        n = int(offsets[r + 1] - offsets[r])
        if _length(np.ma.getdata(fields[r])) != n:
            raise ValueError(f"{what}: radar {r} has {n} gates, its field {_length(np.ma.getdata(fields[r]))}")
        v, m = _host_field(fields[r], _coerce_filters(filters[r]))
        values.append(v)
        masks.append(m)
    return np.concatenate(values), np.concatenate(masks)


def apply_mosaic(geometry: GridGeometry, fields: Sequence, additional_filters: Optional[Sequence] = None,
                 fill_value: float = np.nan) -> np.ndarray:
    """Grid one field of every radar through a mosaic geometry: ``fields[r]`` is radar r's (masked) field in the reference
    format, ``additional_filters[r]`` a list of ``GateFilter`` of radar r.  Returns a float32 grid of
    ``geometry.grid_shape``."""
    offsets = _mosaic_layout(geometry)
    values, mask = _host_concat(offsets, list(fields), additional_filters, "apply_mosaic")
    _check_gather(int(offsets[-1]), 1)
    torch = _native.torch_mod()
    dev = _native.device()
    f_t = torch.from_numpy(values).to(dev)
    m_t = torch.from_numpy(mask).to(dev) if mask.any() else None
    grid = grid_fields_device(geometry, [f_t], [m_t], fill_value=fill_value)
    return _to_host(grid[0]).reshape(geometry.grid_shape)


def apply_mosaic_multi(geometry: GridGeometry, fields: Dict[str, Sequence],
                       additional_filters: Optional[Dict[str, Sequence]] = None,
                       fill_value: float = np.nan) -> Dict[str, np.ndarray]:
    """Several fields of every radar in one pass: ``fields[name][r]`` radar r's field, ``additional_filters[name][r]`` its
    filter list (a missing name: no filters)."""
    offsets = _mosaic_layout(geometry)
    if additional_filters is None:
        additional_filters = {}
    names = list(fields.keys())
    if not names:
        return {}
    host = [_host_concat(offsets, list(fields[n]), additional_filters.get(n), f"apply_mosaic_multi[{n}]") for n in names]
    _check_gather(int(offsets[-1]), len(names))
    torch = _native.torch_mod()
    dev = _native.device()
    f_ts = [torch.from_numpy(v).to(dev) for v, _ in host]
    m_ts = [torch.from_numpy(m).to(dev) if m.any() else None for _, m in host]
    grid = _to_host(grid_fields_device(geometry, f_ts, m_ts, fill_value=fill_value))
    return {name: grid[i].reshape(geometry.grid_shape) for i, name in enumerate(names)}


def _check_gather(n_gates_total: int, n_fields: int) -> None:
    """The geometry route gathers packed fields through a 32-bit buffer resource (rg_csr_apply_f32)."""
    stride = _stride_for(min(n_fields, _native.RG_MAX_FIELDS))
    if n_gates_total * stride * 4 >= _GATHER_BYTES:
        raise ValueError(f"{n_gates_total} gates x {stride} packed slots x 4 bytes reach 4 GiB: too many gates for one "
                         "pass of the geometry route (use a MosaicSearch, or fewer fields per call)")


# ------------------------------------------------------------------------------------------------------------------------
# CSR-free route
# ------------------------------------------------------------------------------------------------------------------------
class MosaicSearch:
    """One :class:`RoiSearch` per radar, each restricted to that radar's reach window (:func:`reach_window`), for
    ``rg_roi_grid_mosaic_f32``.  Radar r's search is ``None`` when it reaches no voxel.  Attributes: ``grid_shape``,
    ``grid_limits``, ``origins`` (float64 ``[R, 3]``), ``n_gates`` (per radar), ``windows``, ``searches``."""

    def __init__(self, radars, grid_shape, grid_limits, min_radius: float = 250.0, beam_factor: float = 0.01746,
                 toa: float = 17000.0, device=None):
        radars = list(radars)
        counts, origins = _check_radars(radars, max_radars=_native.RG_MAX_RADARS)
        self.grid_shape = tuple(int(s) for s in grid_shape)
        if len(self.grid_shape) != 3 or min(self.grid_shape) < 1:
            raise ValueError(f"bad grid shape {grid_shape}")
        self.grid_limits = grid_limits
        self.min_radius = float(min_radius)
        self.beam_factor = float(beam_factor)
        self.toa = toa
        self.origins = origins
        self.n_gates = [int(c) for c in counts]
        self.dev = _native.canonical_device(device)
        self.windows, self.searches = [], []
        for r, (gx, gy, gz, _) in enumerate(radars):
            w = reach_window(gx, gy, gz, self.grid_shape, grid_limits, origins[r], min_radius, beam_factor, toa)
            self.windows.append(w)
            self.searches.append(None if _window_empty(w) else RoiSearch(
                gx, gy, gz, self.grid_shape, mosaic_limits(grid_limits, origins[r]), radar_altitude=0.0,
                min_radius=min_radius, beam_factor=beam_factor, toa=float(toa) - float(origins[r][0]), device=self.dev,
                window=w))

    @classmethod
    def for_path(cls, radars, xs, ys, z_limits, nz, min_radius: float = 250.0, beam_factor: float = 0.01746,
                 toa: float = 17000.0, device=None) -> "MosaicSearch":
        """The search structures of a section along the points ``(xs[i], ys[i])`` (grid frame) with ``nz`` levels over
        ``z_limits``, without a lattice: each radar gets a full-window :class:`RoiSearch` on an ``(nz, 2, 2)`` grid over the
        bounding box of the points in ITS frame, as :func:`vertical_section` builds one for a single radar, so every point
        lies inside every radar's rectangle.  A radar's search is ``None`` exactly when :func:`path_reach` is false for the
        points' bounding box.  (A reach window on a 2 x 2 lattice would not do: a radar lying wholly between the two
        columns has an empty one.)  ``grid_shape`` is ``(nz, 2, 2)``, ``grid_limits`` the points' bounding box."""
        radars = list(radars)
        counts, origins = _check_radars(radars, max_radars=_native.RG_MAX_RADARS)
        xs, ys, limits = _path_limits(xs, ys, z_limits, nz)
        self = cls.__new__(cls)
        self.grid_shape = (int(nz), 2, 2)
        self.grid_limits = limits
        self.min_radius = float(min_radius)
        self.beam_factor = float(beam_factor)
        self.toa = toa
        self.origins = origins
        self.n_gates = [int(c) for c in counts]
        self.dev = _native.canonical_device(device)
        self.windows, self.searches = [], []
        for r, (gx, gy, gz, _) in enumerate(radars):
            search = _path_search(gx, gy, gz, origins[r], xs, ys, nz, limits, min_radius, beam_factor, toa, self.dev)
            self.windows.append((0, 0, 0, 0) if search is None else (0, 2, 0, 2))
            self.searches.append(search)
        return self

    @property
    def n_radars(self) -> int:
        return len(self.searches)

    def table(self, radars: Sequence[int], offsets: Sequence[int]):
        """The ``rg_mosaic_radar`` table of the selected radars, radar ``radars[k]`` at packed offset ``offsets[k]``."""
        table = (_native.MosaicRadar * len(radars))()
        for k, r in enumerate(radars):
            e = table[k]
            e.gate_offset, e.n_gates = int(offsets[k]), self.n_gates[r]
            s = self.searches[r]
            if s is None:
                continue                                          # nx_win = ny_win = 0: never visited
            iy0, iy1, ix0, ix1 = s.window
            e.sorted_gates, e.cell_start, e.cells = _native.ptr(s.sorted_gates), _native.ptr(s.cell_start), s.cells
            e.xc, e.yc, e.zc = _native.ptr(s.xc), _native.ptr(s.yc), _native.ptr(s.zc)
            e.ix0, e.iy0, e.nx_win, e.ny_win = ix0, iy0, ix1 - ix0, iy1 - iy0
        return table

    def section_table(self, radars: Sequence[int], offsets: Sequence[int], points: Sequence):
        """The ``rg_section_radar`` table of the selected radars: radar ``radars[k]`` at packed offset ``offsets[k]`` with
        the points ``points[k] = (xs_t, ys_t)`` in its frame (device tensors the caller keeps alive), or ``None`` where no
        point is the radar's -- such an entry, like one without a search, stays null and takes no part."""
        table = (_native.SectionRadar * len(radars))()
        for k, r in enumerate(radars):
            e = table[k]
            e.gate_offset, e.n_gates = int(offsets[k]), self.n_gates[r]
            s = self.searches[r]
            if s is None or points[k] is None:
                continue
            e.sorted_gates, e.cell_start, e.cells = _native.ptr(s.sorted_gates), _native.ptr(s.cell_start), s.cells
            e.xs, e.ys, e.zc = _native.ptr(points[k][0]), _native.ptr(points[k][1]), _native.ptr(s.zc)
        return table


def _radar_frame(v: np.ndarray, o: float) -> np.ndarray:
    """float32 grid-frame coordinates in the frame of a radar at ``o``: ``fl32(f64(v) - o)``."""
    return (v.astype(np.float64) - float(o)).astype(np.float32)


class _Rectangle:
    """What ``section._check_points`` / ``section_rectangle`` read of a search: the shared grid, unwindowed."""

    def __init__(self, grid_shape, grid_limits):
        self.full_shape = tuple(int(s) for s in grid_shape)
        self.grid_limits = grid_limits
        self.window = (0, self.full_shape[1], 0, self.full_shape[2])


def _path_limits(xs, ys, z_limits, nz):
    """The points as float32 host arrays, validated, and the ``grid_limits`` of their bounding box."""
    if int(nz) < 1:
        raise ValueError(f"nz must be at least 1, not {nz}")
    xs = np.asarray(_host(xs), dtype=np.float32)
    ys = np.asarray(_host(ys), dtype=np.float32)
    box = ((0.0, 0.0), (0.0, 0.0))
    if xs.ndim == 1 and xs.size > 0 and xs.shape == ys.shape and np.all(np.isfinite(xs)) and np.all(np.isfinite(ys)):
        box = ((float(ys.min()), float(ys.max())), (float(xs.min()), float(xs.max())))
    limits = (tuple(float(v) for v in z_limits),) + box
    xs, ys = _check_points(_Rectangle((int(nz), 2, 2), limits), xs, ys, "barnes2")   # raises where the box was not formed
    return xs, ys, limits


def _path_search(gx, gy, gz, origin, xs, ys, nz, limits, min_radius, beam_factor, toa, dev) -> Optional[RoiSearch]:
    """One radar's search structure for the points of a path (``None``: :func:`path_reach` is false): an ``(nz, 2, 2)``
    grid over the bounding box of the points in the radar's frame, its levels those of ``mosaic_limits``."""
    rectangle = (limits[2][0], limits[2][1], limits[1][0], limits[1][1])
    if not path_reach(gx, gy, gz, origin, rectangle, min_radius, beam_factor, toa):
        return None
    x_r, y_r = _radar_frame(xs, origin[2]), _radar_frame(ys, origin[1])
    lim_r = (mosaic_limits(limits, origin)[0], (float(y_r.min()), float(y_r.max())), (float(x_r.min()), float(x_r.max())))
    return RoiSearch(gx, gy, gz, (int(nz), 2, 2), lim_r, radar_altitude=0.0, min_radius=min_radius,
                     beam_factor=beam_factor, toa=float(toa) - float(origin[0]), device=dev)


def _check_device_inputs(fields, masks, shared_masks, counts, n_fields, torch, dev):
    for r, n in enumerate(counts):
        for f, t in enumerate(fields[r]):
            if not (t.is_cuda and t.device == dev and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError(f"radar {r} field {f}: expected a contiguous cuda float32 tensor on {dev}")
        for f, m in enumerate(list(masks[r]) + [shared_masks[r]]):
            if m is not None and not (m.is_cuda and m.device == dev and m.dtype == torch.uint8 and m.is_contiguous()):
                raise ValueError(f"radar {r} mask {f}: expected a contiguous cuda uint8 tensor on {dev}")


def _check_combine(combine: str, return_radar: bool, is_geometry: bool = False) -> None:
    """The combine rule of a CSR-free mosaic call; raises ValueError, touches no device."""
    if combine not in _native.COMBINES:
        raise ValueError(f"Unknown combine rule: {combine} (one of {', '.join(_native.COMBINES)})")
    if return_radar and combine == "mean":
        raise ValueError("return_radar needs combine='max' or 'nearest_radar': a joint mean has no one radar behind it")
    if is_geometry and combine != "mean":
        raise ValueError(f"combine='{combine}' needs a MosaicSearch: a mosaic geometry is one CSR over all radars, a joint "
                         "mean by construction")


def _radar_indices(radar, sel, torch):
    """``out_radar`` of a combine launch (table positions, 255 = none) -> indices of the radars in the MosaicSearch."""
    lut = torch.full((256,), _native.RG_NO_RADAR, dtype=torch.uint8, device=radar.device)
    lut[:len(sel)] = torch.tensor(sel, dtype=torch.uint8, device=radar.device)
    return lut[radar.long()]


def mosaic_fields_device(target, fields: Sequence[Sequence], masks: Optional[Sequence] = None,
                         shared_masks: Optional[Sequence] = None, weighting: str = "barnes2", fill_value: float = np.nan,
                         products=None, radars: Optional[Sequence[int]] = None, combine: str = "mean",
                         return_radar: bool = False):
    """Grid device-resident fields of several radars onto the shared grid.

    ``target``: a mosaic ``GridGeometry`` (:func:`compute_mosaic_geometry`) or a :class:`MosaicSearch`.
    ``fields[k][f]``: cuda float32 tensor of field f of the k-th radar of the call; ``masks[k][f]`` optional uint8 tensors
    (``1`` = excluded), ``shared_masks[k]`` one optional uint8 QC mask of that radar.  ``radars``: which radars of a
    ``MosaicSearch`` the call holds, in that order (default: all) -- any subset; for a geometry it must be all of them, in
    order (its gate numbering is fixed).  ``weighting`` applies to the search route only (a geometry carries its weights).

    ``combine`` (search route only): ``"mean"`` -- the joint weighted mean over the union of every radar's neighbours
    (``rg_roi_grid_mosaic_f32``); ``"max"`` -- per voxel and field the largest of the radars' own means; ``"nearest_radar"``
    -- the mean of the radar whose antenna is closest to the voxel, among those that have one
    (``rg_roi_grid_mosaic_combine_f32``: one launch, no per-radar grids; the rules, ties included, are in
    ``include/radargrid_hip.h``).  A radar's own mean is, bit for bit, what ``radars=[r]`` returns.  ``return_radar=True``
    (not with ``"mean"``) returns ``(grids, radar)``: ``radar`` uint8 ``[F, nz, ny, nx]``, the index in the
    ``MosaicSearch`` of the radar that supplied each value, 255 where the value is the fill.

    Returns ``[F, nz, ny, nx]`` float32, or with a ``PlaneProducts`` what ``grid_products_device`` returns: the geometry
    route goes through ``grid_products_device`` itself (``fused=True`` planes come out of its epilogue), the search route
    grids, then reduces with the separate kernels.  Every argument is validated before the device is touched."""
    is_geometry = isinstance(target, GridGeometry)
    if not is_geometry and not isinstance(target, MosaicSearch):
        raise TypeError("target must be a mosaic GridGeometry or a MosaicSearch")
    _check_combine(combine, return_radar, is_geometry)
    if is_geometry:
        offsets = _mosaic_layout(target)
        n_all = len(offsets) - 1
        all_counts = [int(offsets[r + 1] - offsets[r]) for r in range(n_all)]
        if radars is not None and list(radars) != list(range(n_all)):
            raise ValueError("a mosaic geometry grids all of its radars, in order (its gate numbering is fixed)")
        sel = list(range(n_all))
    else:
        if weighting not in WEIGHTINGS:
            raise ValueError(f"Unknown weighting function: {weighting} (the mosaic has no closest-gate mode)")
        all_counts = target.n_gates
        sel = _select(target.n_radars, radars)
    counts, fields, n_fields, masks, shared_masks, n_total = _check_fields(sel, all_counts, fields, masks, shared_masks)
    if is_geometry:
        _check_gather(n_total, n_fields)

    torch = _native.torch_mod()
    dev = fields[0][0].device
    if dev.type != "cuda":
        raise _native.NativeUnavailable("mosaic_fields_device needs device-resident (cuda) tensors")
    if not is_geometry and dev != target.dev:
        raise ValueError(f"the fields are on {dev}, the MosaicSearch on {target.dev}")
    _check_device_inputs(fields, masks, shared_masks, counts, n_fields, torch, dev)

    with torch.cuda.device(dev):
        cat_fields, cat_field_masks, cat_shared = _concat_on_device(fields, masks, shared_masks, counts, n_fields, torch, dev)
        if is_geometry:
            if products is not None:
                return grid_products_device(target, cat_fields, cat_field_masks, cat_shared, products=products,
                                            fill_value=fill_value)
            return grid_fields_device(target, cat_fields, cat_field_masks, cat_shared, fill_value=fill_value)
        grids, radar = _search_grid(target, sel, counts, cat_fields, cat_field_masks, cat_shared, weighting, fill_value,
                                    dev, combine, return_radar)
    if products is not None:
        grids = ProductPlan(products, target).planes_of_grids(grids)
    return (grids, radar) if return_radar else grids


def _select(n_all: int, radars) -> List[int]:
    """``radars`` (``None``: all) as distinct indices of the ``n_all`` radars of a search; raises ValueError."""
    sel = list(range(n_all)) if radars is None else [int(r) for r in radars]
    if not sel or len(set(sel)) != len(sel) or not all(0 <= r < n_all for r in sel):
        raise ValueError(f"radars must be distinct indices of the {n_all} radars, got {radars!r}")
    return sel


def _check_fields(sel, all_counts, fields, masks, shared_masks):
    """The per-radar fields and masks of a call against the gate counts of the radars ``sel`` -- lengths only, nothing
    touches a device.  Returns ``(counts, fields, n_fields, masks, shared_masks, n_total)`` with the defaults filled in."""
    counts = [all_counts[r] for r in sel]
    fields = [list(f) for f in fields]
    if len(fields) != len(sel):
        raise ValueError(f"expected the fields of {len(sel)} radars, got {len(fields)}")
    n_fields = len(fields[0]) if fields else 0
    if n_fields == 0:
        raise ValueError("no fields to grid")
    masks = [[None] * n_fields for _ in sel] if masks is None else [list(m) for m in masks]
    shared_masks = [None] * len(sel) if shared_masks is None else list(shared_masks)
    if len(masks) != len(sel) or len(shared_masks) != len(sel):
        raise ValueError(f"masks and shared_masks need one entry per radar ({len(sel)})")
    for k, n in enumerate(counts):
        if len(fields[k]) != n_fields:
            raise ValueError(f"radar {sel[k]}: {len(fields[k])} fields, radar {sel[0]} has {n_fields}")
        if len(masks[k]) != n_fields:
            raise ValueError(f"radar {sel[k]}: masks must have one entry (tensor or None) per field")
        for f, t in enumerate(fields[k]):
            if _length(t) != n:
                raise ValueError(f"radar {sel[k]} field {f}: {_length(t)} values for {n} gates")
        for f, m in enumerate(list(masks[k]) + [shared_masks[k]]):
            if m is not None and _length(m) != n:
                raise ValueError(f"radar {sel[k]} mask {f}: {_length(m)} values for {n} gates")
    n_total = sum(counts)
    if n_total > _INT32_MAX:
        raise ValueError(f"{n_total} gates in all: the mosaic numbers gates with int32 (at most 2^31 - 1)")
    return counts, fields, n_fields, masks, shared_masks, n_total


def _concat_on_device(fields, masks, shared_masks, counts, n_fields, torch, dev):
    """The call's radars laid end to end: ``(fields [F], field masks [F] (None where no radar has one), shared mask)``."""
    n_sel = len(counts)

    def cat_masks(pick):
        got = [pick(k) for k in range(n_sel)]
        if all(m is None for m in got):
            return None
        return torch.cat([m if m is not None else torch.zeros(counts[k], dtype=torch.uint8, device=dev)
                          for k, m in enumerate(got)])
    cat_fields = [torch.cat([fields[k][f] for k in range(n_sel)]) for f in range(n_fields)]
    cat_field_masks = [cat_masks(lambda k, f=f: masks[k][f]) for f in range(n_fields)]
    return cat_fields, cat_field_masks, cat_masks(lambda k: shared_masks[k])


def _combine_launcher(entry, name: str, head, weighting, n_total, fill, combine, radar):
    """``pack_and_grid``'s launch callback for a combine entry point: the groups of fields arrive in order, each writes
    its rows of ``radar`` (uint8 ``[F, n_out]``, or ``None``)."""
    done = [0]

    def launch(packed, nf, stride, out_view, stream):
        who = None if radar is None else radar[done[0]:done[0] + nf]
        done[0] += nf
        _native.check(entry(*head, _native.WEIGHTINGS[weighting], _native.ptr(packed), nf, stride, n_total, fill,
                            _native.ptr(out_view), _native.COMBINES[combine], _native.ptr(who), stream), name)
    return launch


def _search_grid(search: MosaicSearch, sel, counts, fields, masks, shared_mask, weighting, fill_value, dev,
                 combine="mean", return_radar=False):
    """``(grids, radar)``; ``radar`` is ``None`` unless asked for."""
    lib = _native.load_library()
    nz, ny, nx = search.grid_shape
    n_total = sum(counts)
    table = search.table(sel, _offsets(counts)[:-1])
    fill = float(np.float32(fill_value))
    if combine == "mean":
        def launch(packed, nf, stride, out_view, stream):
            _native.check(lib.rg_roi_grid_mosaic_f32(
                table, len(sel), nz, ny, nx, search.min_radius, search.beam_factor, _native.WEIGHTINGS[weighting],
                _native.ptr(packed), nf, stride, n_total, fill, _native.ptr(out_view), stream), "rg_roi_grid_mosaic_f32")
        return pack_and_grid(dev, n_total, fields, masks, shared_mask, None, (nz, ny, nx), launch), None
    torch = _native.torch_mod()
    radar = torch.empty((len(fields), nz * ny * nx), dtype=torch.uint8, device=dev) if return_radar else None
    head = (table, len(sel), nz, ny, nx, search.min_radius, search.beam_factor)
    launch = _combine_launcher(lib.rg_roi_grid_mosaic_combine_f32, "rg_roi_grid_mosaic_combine_f32", head, weighting,
                               n_total, fill, combine, radar)
    grids = pack_and_grid(dev, n_total, fields, masks, shared_mask, None, (nz, ny, nx), launch)
    if radar is not None:
        radar = _radar_indices(radar, sel, torch).view(len(fields), nz, ny, nx)
    return grids, radar


# ------------------------------------------------------------------------------------------------------------------------
# a vertical section through a mosaic (csrc/rg_roi_section.hip: rg_roi_section_mosaic_f32)
# ------------------------------------------------------------------------------------------------------------------------
def mosaic_section_points(search: MosaicSearch, xs, ys) -> List[Tuple[np.ndarray, np.ndarray]]:
    """The points ``(xs[i], ys[i])`` -- float32 metres in the shared grid frame -- in every radar's frame: per radar the
    float32 arrays ``(x_r, y_r)`` with ``x_r = fl32(f64(xs) - ox)``, ``y_r = fl32(f64(ys) - oy)``, holding NaN where the
    point lies outside ``section_rectangle(search.searches[r])`` or where radar r has no search.  A NaN point has no
    neighbours among that radar's gates (``rg_roi_section_mosaic_f32``, ``rg_section_count_f32``).

    The points must be finite, one-dimensional, of equal length, at least one, and inside the shared rectangle (the ends
    of the shared grid's float32 coordinate tables); ``ValueError`` otherwise.  Host code: no device is touched.

    For a radar with a non-empty reach window the marking is exact, not an approximation: :func:`reach_window` widens the
    window by one voxel beyond the box of ``gate +- R_g``, so a point beyond the window's rectangle (on a side where the
    window was not cut by the grid, beyond which no point is accepted) lies outside that box and is no gate's neighbour.
    The one limitation: a radar whose lattice window is empty takes no part, as in the lattice mosaic -- on a coarse
    lattice such a radar may still reach points between the columns; :meth:`MosaicSearch.for_path` has no lattice and
    no such case."""
    xs, ys = _check_points(_Rectangle(search.grid_shape, search.grid_limits), xs, ys, "barnes2")
    nan = np.full(xs.shape, np.nan, dtype=np.float32)
    points = []
    for r, s in enumerate(search.searches):
        if s is None:
            points.append((nan.copy(), nan.copy()))
            continue
        x_r, y_r = _radar_frame(xs, search.origins[r][2]), _radar_frame(ys, search.origins[r][1])
        x0, x1, y0, y1 = section_rectangle(s)
        outside = (x_r < x0) | (x_r > x1) | (y_r < y0) | (y_r > y1)
        x_r[outside] = np.nan
        y_r[outside] = np.nan
        points.append((x_r, y_r))
    return points


def _no_closest(weighting: str) -> None:
    if weighting == "closest":
        raise ValueError("weighting 'closest' is a single-radar lattice mode; a mosaic section takes barnes2, cressman or "
                         "nearest")
    if weighting not in WEIGHTINGS:
        raise ValueError(f"Unknown weighting function: {weighting}")


def mosaic_section_fields_device(search: MosaicSearch, xs, ys, fields: Sequence[Sequence], masks: Optional[Sequence] = None,
                                 shared_masks: Optional[Sequence] = None, weighting: str = "barnes2",
                                 fill_value: float = np.nan, radars: Optional[Sequence[int]] = None, combine: str = "mean",
                                 return_radar: bool = False):
    """Grid device-resident fields of several radars at the columns ``(xs[i], ys[i])`` -- float32 metres in the shared grid
    frame, inside the search's rectangle -- straight from the gates (``rg_roi_section_mosaic_f32``): sample ``(k, i)`` is
    the masked weighted mean over the union of every radar's neighbours of the point, each radar in its own frame
    (:func:`mosaic_section_points`).  ``search``: a :class:`MosaicSearch` of a lattice, or of the path itself
    (:meth:`MosaicSearch.for_path`).  ``fields`` / ``masks`` / ``shared_masks`` / ``radars`` as in
    :func:`mosaic_fields_device`; more than ``RG_MAX_FIELDS`` fields go in groups.  Returns ``[F, nz, n_points]`` float32.
    ``combine`` / ``return_radar`` as in :func:`mosaic_fields_device` (``rg_roi_section_mosaic_combine_f32``; ``radar`` is
    uint8 ``[F, nz, n_points]``).  Every argument is validated before the device is touched."""
    if not isinstance(search, MosaicSearch):
        raise TypeError("search must be a MosaicSearch")
    _no_closest(weighting)
    _check_combine(combine, return_radar)
    all_points = mosaic_section_points(search, xs, ys)
    sel = _select(search.n_radars, radars)
    counts, fields, n_fields, masks, shared_masks, n_total = _check_fields(sel, search.n_gates, fields, masks, shared_masks)
    torch = _native.torch_mod()
    dev = fields[0][0].device
    if dev.type != "cuda":
        raise _native.NativeUnavailable("mosaic_section_fields_device needs device-resident (cuda) tensors")
    if dev != search.dev:
        raise ValueError(f"the fields are on {dev}, the MosaicSearch on {search.dev}")
    _check_device_inputs(fields, masks, shared_masks, counts, n_fields, torch, dev)
    lib = _native.load_library()
    nz, n_points = search.grid_shape[0], int(all_points[0][0].size)
    fill = float(np.float32(fill_value))
    with torch.cuda.device(dev):
        cat_fields, cat_field_masks, cat_shared = _concat_on_device(fields, masks, shared_masks, counts, n_fields, torch, dev)
        # the points of a radar that serves at least one of them, on the device
        points = [None if np.isnan(all_points[r][0]).all() else
                  (torch.from_numpy(all_points[r][0]).to(dev), torch.from_numpy(all_points[r][1]).to(dev)) for r in sel]
        table = search.section_table(sel, _offsets(counts)[:-1], points)

        if combine == "mean":
            def launch(packed, nf, stride, out_view, stream):
                _native.check(lib.rg_roi_section_mosaic_f32(
                    table, len(sel), nz, n_points, search.min_radius, search.beam_factor, _native.WEIGHTINGS[weighting],
                    _native.ptr(packed), nf, stride, n_total, fill, _native.ptr(out_view), stream),
                    "rg_roi_section_mosaic_f32")
            return pack_and_grid(dev, n_total, cat_fields, cat_field_masks, cat_shared, None, (nz, n_points), launch)
        radar = torch.empty((n_fields, nz * n_points), dtype=torch.uint8, device=dev) if return_radar else None
        head = (table, len(sel), nz, n_points, search.min_radius, search.beam_factor)
        launch = _combine_launcher(lib.rg_roi_section_mosaic_combine_f32, "rg_roi_section_mosaic_combine_f32", head,
                                   weighting, n_total, fill, combine, radar)
        out = pack_and_grid(dev, n_total, cat_fields, cat_field_masks, cat_shared, None, (nz, n_points), launch)
        if radar is None:
            return out
        return out, _radar_indices(radar, sel, torch).view(n_fields, nz, n_points)


def compute_mosaic_section_geometry(radars, xs, ys, z_limits, nz, min_radius: float = 250.0, beam_factor: float = 0.01746,
                                    weighting: str = "barnes2", toa: float = 17000.0) -> GridGeometry:
    """The CSR of a section through a mosaic as an ordinary geometry of ``grid_shape (nz, 1, n_points)``: row
    ``k * n_points + i`` is radar 0's row -- the gates within the radius of influence of ``(xs[i], ys[i], z_k)`` in radar
    0's frame, float64-exact weights rounded to float32 -- then radar 1's, and so on, with radar r's gate g numbered
    ``gate_offsets[r] + g``.  Any number of radars: each is counted and filled on its own (``rg_section_count_f32`` /
    ``rg_section_fill_f32`` over a search built as :meth:`MosaicSearch.for_path` builds it), a running cursor placing its
    segment of every row.  The result carries ``.gate_offsets``, ``.origins``, ``.section_x``, ``.section_y`` and goes
    through :func:`apply_mosaic`, :func:`apply_mosaic_multi`, :func:`mosaic_fields_device` and ``save_geometry`` like a
    lattice mosaic geometry."""
    _no_closest(weighting)
    radars = list(radars)
    counts, origins = _check_radars(radars)
    xs, ys, limits = _path_limits(xs, ys, z_limits, nz)
    nz, n_points = int(nz), int(xs.size)
    n_rows = nz * n_points
    offsets = _offsets(counts)
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _native.device()
    from .section import _section_args
    with torch.cuda.device(dev):
        stream = _native.stream_ptr()
        parts = []        # per radar that reaches the path: (r, search, the ten leading arguments, its points, its row lengths)
        total = torch.zeros(n_rows + 1, dtype=torch.int32, device=dev)
        for r, (gx, gy, gz, _) in enumerate(radars):
            search = _path_search(gx, gy, gz, origins[r], xs, ys, nz, limits, min_radius, beam_factor, toa, dev)
            if search is None:
                continue
            pts = (torch.from_numpy(_radar_frame(xs, origins[r][2])).to(dev),
                   torch.from_numpy(_radar_frame(ys, origins[r][1])).to(dev))
            head = _section_args(search, *pts)
            row_counts = torch.zeros(n_rows + 1, dtype=torch.int32, device=dev)
            _native.check(lib.rg_section_count_f32(*head, _native.ptr(row_counts), stream), "rg_section_count_f32")
            total += row_counts
            parts.append((r, search, head, pts, row_counts))

        def fill(indptr, gate_idx, weights):
            # running cursor: the fill kernel reads only cursor[row] as the row base and writes at absolute positions
            cursor = indptr[:n_rows].clone()
            for r, search, head, _, row_counts in parts:
                # the radar's gate numbers carry its offset: shift the index column of this build's copy of its sorted gates
                search.sorted_gates.view(torch.int32).view(-1, 4)[:, 3] += int(offsets[r])
                _native.check(lib.rg_section_fill_f32(*head, _native.WEIGHTINGS[weighting], _native.ptr(cursor),
                                                      _native.ptr(gate_idx), _native.ptr(weights), stream),
                              "rg_section_fill_f32")
                cursor += row_counts[:n_rows]
        csr = csr_from_counts(total, n_rows, fill)
        del parts
    z_lim = tuple(float(v) for v in z_limits)
    geom = GridGeometry.from_device((nz, 1, n_points), (z_lim, (0.0, 0.0), (0.0, _cumulative_distance(xs, ys))), csr, toa)
    geom.gate_offsets = offsets
    geom.origins = origins
    geom.section_x, geom.section_y = xs, ys
    return geom


def mosaic_vertical_section(radars, fields: Sequence, vertices, spacing, z_limits, nz, additional_filters=None,
                            min_radius: float = 250.0, beam_factor: float = 0.01746, weighting: str = "barnes2",
                            toa: float = 17000.0, fill_value: float = np.nan, combine: str = "mean"):
    """One masked field of every radar on the vertical section along the polyline ``vertices`` (grid frame) sampled every
    ``spacing`` metres (:func:`section_path`), ``nz`` levels over ``z_limits``: NumPy in, NumPy out.  ``radars``:
    ``[(gate_x, gate_y, gate_z, origin), ...]``, at most ``RG_MAX_RADARS``; ``fields[r]`` radar r's (masked) field in the
    reference format, ``additional_filters[r]`` its list of ``GateFilter``.  Returns ``(section float32 [nz, n_points],
    s float64 [n_points])`` -- :func:`mosaic_section_fields_device` on :meth:`MosaicSearch.for_path`, with its ``combine``
    rule (``"mean"``, ``"max"`` or ``"nearest_radar"``)."""
    xs, ys, s = section_path(vertices, spacing)
    _no_closest(weighting)
    _check_combine(combine, False)
    radars = list(radars)
    counts, _ = _check_radars(radars, max_radars=_native.RG_MAX_RADARS)
    fields = list(fields)
    if additional_filters is None:
        additional_filters = [None] * len(radars)
    if len(fields) != len(radars) or len(additional_filters) != len(radars):
        raise ValueError(f"mosaic_vertical_section: expected one field and one filter list per radar ({len(radars)})")
    host = []
    for r, n in enumerate(counts):
        v, m = _host_field(fields[r], _coerce_filters(additional_filters[r]))
        if v.size != n:
            raise ValueError(f"mosaic_vertical_section: radar {r} has {n} gates, its field {v.size}")
        host.append((v, m))
    search = MosaicSearch.for_path(radars, xs, ys, z_limits, nz, min_radius, beam_factor, toa)
    torch = _native.torch_mod()
    f_ts = [[torch.from_numpy(v).to(search.dev)] for v, _ in host]
    m_ts = [[torch.from_numpy(m).to(search.dev) if m.any() else None] for _, m in host]
    out = mosaic_section_fields_device(search, xs, ys, f_ts, m_ts, weighting=weighting, fill_value=fill_value,
                                       combine=combine)
    return _to_host(out[0]), s
