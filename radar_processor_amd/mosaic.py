"""Several radars on one shared grid (mosaic).

Each radar gives float32 gate coordinates relative to its antenna (what ``get_gate_coordinates`` returns) and its
``origin = (oz, oy, ox)``: the antenna position in the grid frame, in metres, in the axis order of ``grid_limits``.  Gates
are translated into the grid frame, not rotated or re-projected.  Radars that stand apart need the re-projection first:
``georef.place_radar`` / ``place_radars`` make the tuple from each radar's longitude, latitude and altitude.

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
  (``rg_roi_grid_mosaic_combine_f32``; its joint mean is the kernel of ``rg_roi_grid_mosaic_f32``) -- no CSR, any subset
  of the radars per call.

A vertical section through a mosaic (``csrc/rg_roi_section.hip``: ``rg_roi_section_mosaic_f32``) has the same two routes:
:func:`mosaic_section_fields_device` on a :class:`MosaicSearch` -- of a lattice, or of the path itself
(:meth:`MosaicSearch.for_path`) -- and :func:`compute_mosaic_section_geometry`; :func:`mosaic_vertical_section` is the
NumPy-in / NumPy-out convenience.  The points are given in the grid frame and seen from every radar's own frame
(:func:`mosaic_section_points`).
"""
from __future__ import annotations

import math
import os
from typing import Callable, Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _native
from .geometry_builder import _INT32_MAX, WEIGHTINGS, RoiSearch, csr_from_counts
from .grid_geometry import GridGeometry
from .gridding import _coerce_filters, _host_field, _stride_for, _to_host, grid_fields_device
from .plane_products import ProductPlan, grid_products_device
from .roi_grid import pack_and_grid
from .section import (_PathRows, _check_points_in, _refuse_closest, _cumulative_distance, _grid_rectangle, _host,
                      _length, _upload, section_path, section_rectangle)

_GATHER_BYTES = 2 ** 32        # buffer-resource range of the packed-field gather in rg_csr_apply_f32
MOSAIC_COMBINES = tuple(_native.COMBINES)      # "mean", "max", "nearest_radar": the combine rules of the CSR-free route
NO_RADAR = _native.RG_NO_RADAR                 # in a ``radar`` map: no radar has a value there (the grid holds the fill)


def mosaic_limits(grid_limits, origin) -> Tuple[Tuple[float, float], ...]:
    """The shared grid's limits in the frame of a radar at ``origin = (oz, oy, ox)`` (Python floats)."""
    return tuple((float(lo) - float(o), float(hi) - float(o)) for (lo, hi), o in zip(grid_limits, origin))


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


def _window_searches(radars, origins, grid_shape, grid_limits, min_radius, beam_factor, toa, dev):
    """Per radar its reach window on the shared grid and its :class:`RoiSearch` over that window, in its own frame
    (``None``: the window is empty): ``(windows, searches)``."""
    windows, searches = [], []
    for (gx, gy, gz, _), origin in zip(radars, origins):
        w = reach_window(gx, gy, gz, grid_shape, grid_limits, origin, min_radius, beam_factor, toa)
        windows.append(w)
        searches.append(None if _window_empty(w) else RoiSearch(
            gx, gy, gz, grid_shape, mosaic_limits(grid_limits, origin), radar_altitude=0.0, min_radius=min_radius,
            beam_factor=beam_factor, toa=float(toa) - float(origin[0]), device=dev, window=w))
    return windows, searches


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
    _native.load_library()
    dev = _native.device()
    shape = nz, ny, nx = tuple(int(s) for s in grid_shape)

    def part(r, search):
        iy0, iy1, ix0, ix1 = search.window
        return _RowsPart(r, search, lambda rows: rows.view(nz, ny, nx)[:, iy0:iy1, ix0:ix1],
                         lambda: search.count_rows()[:-1].view(search.grid_shape),
                         lambda base, gate_idx, weights: search.fill_rows(weighting, _native.ptr(base), _native.ptr(gate_idx),
                                                                          _native.ptr(weights)))
    # per radar that reaches a voxel: its search over its reach window, all of them built before the first count
    searches = _window_searches(radars, origins, shape, grid_limits, min_radius, beam_factor, toa, dev)[1]
    return _stacked_geometry(shape, grid_limits, toa, counts, origins,
                             [part(r, search) for r, search in enumerate(searches) if search is not None], dev)


class _RowsPart(NamedTuple):
    """One radar's share of a stacked CSR (:func:`_stacked_geometry`)."""
    radar: int              # its index: its gates are numbered from gate_offsets[radar]
    search: RoiSearch       # this build's own: the index column of its sorted gates gets the offset
    rows: Callable          # a tensor over the shared rows -> the view of the rows this radar serves, in its own order
    count: Callable         # () -> int32 neighbour counts, shaped like that view
    fill: Callable          # (base, gate_idx, weights): write its pairs of row v from position base[v] (contiguous) on


def _stacked_geometry(grid_shape, grid_limits, toa, counts, origins, parts: Iterable[_RowsPart], dev) -> GridGeometry:
    """The one row-stacking builder: the CSR whose row v is the first part's row v, then the second's, and so on, as a
    mosaic geometry (``.gate_offsets``, ``.origins``).  ``parts`` may be a generator: a part is counted as it arrives."""
    torch = _native.torch_mod()
    n_rows = int(np.prod(grid_shape))
    offsets = _offsets(counts)
    with torch.cuda.device(dev):
        total = torch.zeros(n_rows + 1, dtype=torch.int32, device=dev)
        counted = []
        for p in parts:
            counted.append((p, p.count()))
            p.rows(total[:n_rows]).add_(counted[-1][1])

        def fill(indptr, gate_idx, weights):
            # running cursor: indptr plus the counts of the radars already filled.  The fill kernels read only cursor[v] as
            # the row base and write at absolute positions, so every radar fills its segment of each of its rows.
            cursor = indptr[:n_rows].clone()
            for p, n in counted:
                base = p.rows(cursor).contiguous()
                # the radar's gate numbers carry its offset: shift the index column of this build's copy of its sorted gates
                p.search.sorted_gates.view(torch.int32).view(-1, 4)[:, 3] += int(offsets[p.radar])
                p.fill(base, gate_idx, weights)
                p.rows(cursor).add_(n)
        csr = csr_from_counts(total, n_rows, fill)
    geom = GridGeometry.from_device(grid_shape, grid_limits, csr, toa)
    geom.gate_offsets = offsets
    geom.origins = origins
    return geom


def _mosaic_layout(geometry) -> np.ndarray:
    offsets = getattr(geometry, "gate_offsets", None)
    if offsets is None:
        raise ValueError("not a mosaic: the geometry has no gate_offsets (built by compute_mosaic_geometry)")
    return np.asarray(offsets, dtype=np.int64)


def _host_fields(counts, fields, filters, what: str):
    """The one intake of host fields: radar r's masked field ``fields[r]`` and its list of ``GateFilter`` ``filters[r]``
    (``filters`` ``None``: none) -> ``[(values float32, mask uint8), ...]``, each checked against the radar's gate count."""
    host = []
    for r, n in enumerate(counts):
        size = _length(np.ma.getdata(fields[r]))
        if size != int(n):
            raise ValueError(f"{what}: radar {r} has {int(n)} gates, its field {size}")
        host.append(_host_field(fields[r], _coerce_filters(None if filters is None else filters[r])))
    return host


def _apply_through(geometry, fields: Dict[str, Sequence], filters: Dict[str, Sequence], fill_value, what: str):
    """``apply_mosaic_multi`` proper: every named field's radars laid end to end, uploaded, one pass through the geometry."""
    offsets = _mosaic_layout(geometry)
    if not fields:
        return {}
    n_radars = len(offsets) - 1
    cat = []
    for name, per_radar in fields.items():
        label, per_radar, flt = what.format(name), list(per_radar), filters.get(name)
        if len(per_radar) != n_radars:
            raise ValueError(f"{label}: expected one field per radar ({n_radars}), got {len(per_radar)}")
        if flt is not None and len(flt) != n_radars:
            raise ValueError(f"{label}: expected one filter list per radar ({n_radars}), got {len(flt)}")
        host = _host_fields(np.diff(offsets), per_radar, flt, label)
        cat.append((np.concatenate([v for v, _ in host]), np.concatenate([m for _, m in host])))
    _check_gather(int(offsets[-1]), len(cat))
    on_device = [_upload(v, m, _native.device()) for v, m in cat]
    grid = _to_host(grid_fields_device(geometry, [f for f, _ in on_device], [m for _, m in on_device], fill_value=fill_value))
    return {name: grid[i].reshape(geometry.grid_shape) for i, name in enumerate(fields)}


def apply_mosaic(geometry: GridGeometry, fields: Sequence, additional_filters: Optional[Sequence] = None,
                 fill_value: float = np.nan) -> np.ndarray:
    """Grid one field of every radar through a mosaic geometry: ``fields[r]`` is radar r's (masked) field in the reference
    format, ``additional_filters[r]`` a list of ``GateFilter`` of radar r.  Returns a float32 grid of
    ``geometry.grid_shape``."""
    return _apply_through(geometry, {"": fields}, {"": additional_filters}, fill_value, "apply_mosaic")[""]


def apply_mosaic_multi(geometry: GridGeometry, fields: Dict[str, Sequence],
                       additional_filters: Optional[Dict[str, Sequence]] = None,
                       fill_value: float = np.nan) -> Dict[str, np.ndarray]:
    """Several fields of every radar in one pass: ``fields[name][r]`` radar r's field, ``additional_filters[name][r]`` its
    filter list (a missing name: no filters)."""
    return _apply_through(geometry, fields, additional_filters or {}, fill_value, "apply_mosaic_multi[{}]")


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
        shape = tuple(int(s) for s in grid_shape)
        if len(shape) != 3 or min(shape) < 1:
            raise ValueError(f"bad grid shape {grid_shape}")
        dev = _native.canonical_device(device)
        self._set(shape, grid_limits, min_radius, beam_factor, toa, origins, counts, dev,
                  *_window_searches(radars, origins, shape, grid_limits, min_radius, beam_factor, toa, dev))

    def _set(self, grid_shape, grid_limits, min_radius, beam_factor, toa, origins, counts, dev, windows, searches) -> None:
        """The one place that sets a MosaicSearch's attributes, from values either constructor has prepared."""
        self.grid_shape = grid_shape
        self.grid_limits = grid_limits
        self.min_radius = float(min_radius)
        self.beam_factor = float(beam_factor)
        self.toa = toa
        self.origins = origins
        self.n_gates = [int(c) for c in counts]
        self.dev = dev
        self.windows, self.searches = windows, searches

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
        dev = _native.canonical_device(device)
        searches = [_path_search(gx, gy, gz, origins[r], xs, ys, nz, limits, min_radius, beam_factor, toa, dev)
                    for r, (gx, gy, gz, _) in enumerate(radars)]
        self = cls.__new__(cls)
        self._set((int(nz), 2, 2), limits, min_radius, beam_factor, toa, origins, counts, dev,
                  [(0, 0, 0, 0) if s is None else (0, 2, 0, 2) for s in searches], searches)
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
    xs, ys = _check_points_in(_grid_rectangle((int(nz), 2, 2), limits), xs, ys)     # raises where the box was not formed
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
    (the kernel of ``rg_roi_grid_mosaic_f32``); ``"max"`` -- per voxel and field the largest of the radars' own means;
    ``"nearest_radar"`` -- the mean of the radar whose antenna is closest to the voxel, among those that have one
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
    if not is_geometry:
        _refuse_closest(weighting, "a mosaic")
    call = _prepare(target, fields, masks, shared_masks, radars, "mosaic_fields_device")
    if is_geometry:
        with _native.torch_mod().cuda.device(call.dev):
            if products is not None:
                return grid_products_device(target, call.fields, call.masks, call.shared_mask, products=products,
                                            fill_value=fill_value)
            return grid_fields_device(target, call.fields, call.masks, call.shared_mask, fill_value=fill_value)
    nz, ny, nx = target.grid_shape
    head = (target.table(call.sel, call.offsets), len(call.sel), nz, ny, nx, target.min_radius, target.beam_factor)
    grids, radar = _launch(call, "rg_roi_grid_mosaic_combine_f32", head, (nz, ny, nx), weighting, fill_value, combine,
                           return_radar)
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


class _Call(NamedTuple):
    """A validated CSR-free call (:func:`_prepare`): what a launch needs besides its table."""
    sel: List[int]            # the radars of the call: indices into the MosaicSearch (or all of a geometry's)
    counts: List[int]         # their gate counts
    n_total: int
    dev: object
    fields: list              # [F] tensors, the call's radars laid end to end
    masks: list               # [F] tensors or None
    shared_mask: object
    offsets: np.ndarray       # radar sel[k]'s first gate in those tensors


def _prepare(target, fields, masks, shared_masks, radars, who: str) -> _Call:
    """The one route from the arguments of a device call to its launches: the radars of the call (``radars`` of a
    :class:`MosaicSearch`, all of a mosaic geometry), every length, the device, every tensor -- then the call's radars
    concatenated on the device.  Nothing touches the device before every check has passed."""
    if isinstance(target, MosaicSearch):
        all_counts, sel = target.n_gates, _select(target.n_radars, radars)
    else:
        all_counts = np.diff(_mosaic_layout(target)).tolist()
        sel = list(range(len(all_counts)))
        if radars is not None and list(radars) != sel:
            raise ValueError("a mosaic geometry grids all of its radars, in order (its gate numbering is fixed)")
    counts, fields, n_fields, masks, shared_masks, n_total = _check_fields(sel, all_counts, fields, masks, shared_masks)
    if not isinstance(target, MosaicSearch):
        _check_gather(n_total, n_fields)
    torch = _native.torch_mod()
    dev = fields[0][0].device
    if dev.type != "cuda":
        raise _native.NativeUnavailable(f"{who} needs device-resident (cuda) tensors")
    if isinstance(target, MosaicSearch) and dev != target.dev:
        raise ValueError(f"the fields are on {dev}, the MosaicSearch on {target.dev}")
    _check_device_inputs(fields, masks, shared_masks, counts, n_fields, torch, dev)
    with torch.cuda.device(dev):
        cat = _concat_on_device(fields, masks, shared_masks, counts, n_fields, torch, dev)
    return _Call(sel, counts, n_total, dev, *cat, _offsets(counts)[:-1])


def _launch(call: _Call, entry: str, head: tuple, out_shape: tuple, weighting, fill_value, combine, return_radar):
    """The one launcher of the CSR-free mosaic calls: ``call`` through the combine entry point ``entry`` of the lattice or
    of the section (``head``: its arguments up to the weighting, the table first) under any of the three rules -- the
    joint mean is ``RG_COMBINE_MEAN`` with a null ``out_radar``, the kernel of the mean entry points.  Returns ``(out
    [F, *out_shape], radar)``; ``radar`` (``return_radar``, else ``None``) uint8 of that shape: indices into the
    MosaicSearch, ``pack_and_grid``'s groups of fields having written their rows of it one after the other."""
    torch = _native.torch_mod()
    launch_entry = getattr(_native.load_library(), entry)
    fill = float(np.float32(fill_value))
    n_fields = len(call.fields)
    radar = torch.empty((n_fields, math.prod(out_shape)), dtype=torch.uint8, device=call.dev) if return_radar else None
    done = [0]

    def launch(packed, nf, stride, out_view, stream):
        who = None if radar is None else radar[done[0]:done[0] + nf]
        done[0] += nf
        _native.check(launch_entry(*head, _native.WEIGHTINGS[weighting], _native.ptr(packed), nf, stride, call.n_total,
                                   fill, _native.ptr(out_view), _native.COMBINES[combine], _native.ptr(who), stream), entry)
    out = pack_and_grid(call.dev, call.n_total, call.fields, call.masks, call.shared_mask, None, out_shape, launch)
    if radar is not None:           # table positions (255 = none) -> indices of the radars in the MosaicSearch
        lut = torch.full((256,), _native.RG_NO_RADAR, dtype=torch.uint8, device=call.dev)
        lut[:len(call.sel)] = torch.tensor(call.sel, dtype=torch.uint8, device=call.dev)
        radar = lut[radar.long()].view((n_fields,) + tuple(out_shape))
    return out, radar


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
    xs, ys = _check_points_in(_grid_rectangle(search.grid_shape, search.grid_limits), xs, ys)
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
    _refuse_closest(weighting, "a mosaic section")
    _check_combine(combine, return_radar)
    all_points = mosaic_section_points(search, xs, ys)
    call = _prepare(search, fields, masks, shared_masks, radars, "mosaic_section_fields_device")
    # the points of a radar that serves at least one of them, on the device
    torch = _native.torch_mod()
    points = [None if np.isnan(all_points[r][0]).all() else
              (torch.from_numpy(all_points[r][0]).to(call.dev), torch.from_numpy(all_points[r][1]).to(call.dev))
              for r in call.sel]
    nz, n_points = search.grid_shape[0], int(all_points[0][0].size)
    head = (search.section_table(call.sel, call.offsets, points), len(call.sel), nz, n_points, search.min_radius,
            search.beam_factor)
    out, radar = _launch(call, "rg_roi_section_mosaic_combine_f32", head, (nz, n_points), weighting, fill_value, combine,
                         return_radar)
    return (out, radar) if return_radar else out


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
    _refuse_closest(weighting, "a mosaic section")
    radars = list(radars)
    counts, origins = _check_radars(radars)
    xs, ys, limits = _path_limits(xs, ys, z_limits, nz)
    _native.load_library()
    dev = _native.device()

    def parts():        # per radar that reaches the path: its search is built, then counted, before the next radar's
        for r, (gx, gy, gz, _) in enumerate(radars):
            search = _path_search(gx, gy, gz, origins[r], xs, ys, nz, limits, min_radius, beam_factor, toa, dev)
            if search is not None:
                rows = _PathRows(search, _radar_frame(xs, origins[r][2]), _radar_frame(ys, origins[r][1]))
                yield _RowsPart(r, search, lambda shared: shared, lambda rows=rows: rows.count()[:-1],
                                lambda *csr_arrays, rows=rows: rows.fill(weighting, *csr_arrays))
    z_lim = tuple(float(v) for v in z_limits)
    geom = _stacked_geometry((int(nz), 1, int(xs.size)), (z_lim, (0.0, 0.0), (0.0, _cumulative_distance(xs, ys))), toa,
                             counts, origins, parts(), dev)
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
    _refuse_closest(weighting, "a mosaic section")
    _check_combine(combine, False)
    radars, fields = list(radars), list(fields)
    counts, _ = _check_radars(radars, max_radars=_native.RG_MAX_RADARS)
    if len(fields) != len(radars) or (additional_filters is not None and len(additional_filters) != len(radars)):
        raise ValueError(f"mosaic_vertical_section: expected one field and one filter list per radar ({len(radars)})")
    host = _host_fields(counts, fields, additional_filters, "mosaic_vertical_section")
    search = MosaicSearch.for_path(radars, xs, ys, z_limits, nz, min_radius, beam_factor, toa)
    on_device = [_upload(v, m, search.dev) for v, m in host]
    out = mosaic_section_fields_device(search, xs, ys, [[f] for f, _ in on_device], [[m] for _, m in on_device],
                                       weighting=weighting, fill_value=fill_value, combine=combine)
    return _to_host(out[0]), s
