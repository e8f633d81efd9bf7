"""Following storm cells from frame to frame (include/radargrid_hip.h, "Cell overlap and tracking"; kernels in
csrc/rg_tracking.hip): which cell of the new frame is which cell of the old one.

* :func:`advect_labels_device` moves the earlier frame's labels to the later frame's time along a motion field;
* :func:`cell_overlap_device` counts, for every pair (old cell, new cell), the pixels they share (``rg_cell_overlap_i32``);
* :func:`match_cells` picks each cell's successor and predecessor from those counts (host NumPy, a few hundred pairs);
* :func:`relabel_cells_device` maps a label plane to any per-cell integer (``rg_relabel_cells_i32``);
* :class:`CellTracker` chains them with :mod:`components` and :mod:`motion` and keeps track ids, ages, velocities, splits and
  merges.

Cells are addressed by their ROW in a :class:`~radar_processor_amd.components.CellTable` (``cell_ptr[p] + id - 1``).  The device
functions take tensors or ndarrays, enqueue on torch's current stream and validate every argument before the device is
touched.  :func:`cell_overlap_device` synchronises with the host once, to read ``totals`` (and once more, before the launch,
when it has to size the table itself).
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np

from . import _native
from . import components as _cc
from . import motion as _mo

MAX_PAIRS_LIMIT = 2 ** 30           # rg_cell_overlap_i32 takes 1 <= max_pairs < 2^30


class CellOverlap(NamedTuple):
    """The pairs of cells that share pixels, sorted by ``(row_prev, row_next)``: int32 device tensors of one length."""
    row_prev: object         # row of the cell in the earlier frame's table
    row_next: object         # row of the cell in the later frame's table
    count: object            # pixels the two share


class CellMatch(NamedTuple):
    """What :func:`match_cells` returns (host arrays).  ``succ[a]``: the row of the later frame that cell ``a`` of the earlier
    frame goes to, ``-1`` for none; ``pred[b]``: where cell ``b`` of the later frame comes from.  ``row_prev``, ``row_next``,
    ``count``: the qualifying pairs, in the overlap's order."""
    succ: np.ndarray         # int64 [cells of the earlier frame]
    pred: np.ndarray         # int64 [cells of the later frame]
    row_prev: np.ndarray     # int32
    row_next: np.ndarray     # int32
    count: np.ndarray        # int32


# ---- validation (host only) --------------------------------------------------------------------------------------------------
def _is_tensor(a) -> bool:
    return type(a).__module__.startswith("torch")


def _dtype_name(a) -> str:
    return str(a.dtype).replace("torch.", "")


def _is_int(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def _check_labels(labels, what: str):
    """``(n, h, w)`` of int32 ``[h, w]`` or ``[n, h, w]`` labels (tensor or ndarray), by dtype and rank only."""
    if not hasattr(labels, "shape") or not hasattr(labels, "dtype"):
        raise ValueError(f"{what} must be a tensor or an ndarray, not {type(labels).__name__}")
    shape = tuple(int(n) for n in labels.shape)
    if _dtype_name(labels) != "int32" or len(shape) not in (2, 3):
        raise ValueError(f"{what} must be int32 [h, w] or [n, h, w]; got {_dtype_name(labels)} {list(shape)}")
    shape3 = (1,) + shape if len(shape) == 2 else shape
    if shape3[0] < 1:
        raise ValueError(f"{what}: no planes in shape {list(shape)}")
    if shape3[0] * shape3[1] * shape3[2] >= 2 ** 31:
        raise ValueError(f"{what}: {list(shape)} holds 2^31 pixels or more")
    return shape3


def _check_cell_ptr(cell_ptr, n: int, what: str) -> None:
    if not hasattr(cell_ptr, "shape") or _dtype_name(cell_ptr) != "int32" or tuple(int(v) for v in cell_ptr.shape) != (n + 1,):
        raise ValueError(f"{what} must be int32 [{n + 1}] for {n} plane(s); got "
                         f"{getattr(cell_ptr, 'dtype', type(cell_ptr).__name__)} {list(getattr(cell_ptr, 'shape', []))}")


def _check_max_pairs(max_pairs) -> Optional[int]:
    if max_pairs is None:
        return None
    if not _is_int(max_pairs) or not 1 <= max_pairs < MAX_PAIRS_LIMIT:
        raise ValueError(f"max_pairs must be an integer in 1 .. 2^30 - 1 or None, not {max_pairs!r}")
    return int(max_pairs)


def _check_match_limits(min_pixels, min_fraction):
    if not _is_int(min_pixels) or min_pixels < 1:
        raise ValueError(f"min_pixels must be an integer of at least 1, not {min_pixels!r}")
    try:
        fraction = float(min_fraction)
    except (TypeError, ValueError):
        fraction = float("nan")
    if not 0.0 <= fraction <= 1.0:
        raise ValueError(f"min_fraction must lie in 0 .. 1, not {min_fraction!r}")
    return int(min_pixels), fraction


def _host(a, dtype=None) -> np.ndarray:
    a = a.detach().cpu().numpy() if _is_tensor(a) else np.asarray(a)
    return a if dtype is None else a.astype(dtype, copy=False)


# ---- device ------------------------------------------------------------------------------------------------------------------
def advect_labels_device(labels, motion, *, lattice=None, lead: float = 1.0, substeps: int = 1):
    """int32 labels ``[h, w]`` of the earlier frame moved along ``motion`` by ``lead`` intervals: the label that sits at
    ``floor(p - d + 0.5)`` for every pixel ``p``, 0 where that lies outside the plane.

    No kernel of its own: :func:`~radar_processor_amd.motion.advect_device` with ``method="nearest"`` copies 32 bits per pixel
    whatever they mean, so the labels go through it viewed as float32, with the fill's bits 0.  ``motion``, ``lattice`` and
    ``substeps`` as there; lead 0 returns the labels' bytes."""
    shape3 = _check_labels(labels, "labels")
    if len(labels.shape) != 2:
        raise ValueError(f"labels must be ONE int32 [h, w] plane, got {list(labels.shape)}")
    try:
        lead = float(lead)
    except (TypeError, ValueError):
        raise ValueError(f"lead must be a number in units of the interval, got {lead!r}") from None
    _mo._check_field(motion, lattice, shape3[1:])
    _mo._check_leads((lead,))
    _mo._check_sampling("nearest", substeps, 0.0, None, shape3)
    torch = _native.torch_mod()
    if not _is_tensor(labels):
        labels = torch.from_numpy(np.array(labels, dtype=np.int32))              # a copy: torch takes no read-only array
    bits = labels.contiguous().view(torch.float32)
    out = _mo.advect_device(bits, motion, (lead,), lattice=lattice, method="nearest", substeps=substeps, fill_value=0.0)
    return out[0].view(torch.int32)


def cell_overlap_device(labels_prev, cell_ptr_prev, labels_next, cell_ptr_next, *, max_pairs: Optional[int] = None) -> CellOverlap:
    """The pixels every pair (cell of ``labels_prev``, cell of ``labels_next``) shares (``rg_cell_overlap_i32``).

    ``labels_*`` int32 ``[h, w]`` or ``[n, h, w]`` of one shape with their ``cell_ptr_*`` int32 ``[n + 1]``, as
    :func:`~radar_processor_amd.components.label_components_device` returns them; plane ``p`` is paired with plane ``p`` (the
    two may be ``L[:-1]`` and ``L[1:]`` of one stack).  Returns a :class:`CellOverlap` sorted by ``(row_prev, row_next)`` -- the
    sort is a ``torch.sort`` over the few pairs that exist.

    ``max_pairs`` sizes the hash table (twice that many slots) and the outputs.  ``None``: ``max(1, min(pixels, cells_prev *
    cells_next))``, which always suffices and costs one read of the two cell counts.  The function reads ``totals`` once --
    its host synchronisation -- and raises ``RuntimeError`` when an explicit ``max_pairs`` was too small."""
    shape3 = _check_labels(labels_prev, "labels_prev")
    if _check_labels(labels_next, "labels_next") != shape3 or tuple(labels_prev.shape) != tuple(labels_next.shape):
        raise ValueError(f"labels_prev of shape {list(labels_prev.shape)} and labels_next of shape {list(labels_next.shape)} differ")
    n, h, w = shape3
    _check_cell_ptr(cell_ptr_prev, n, "cell_ptr_prev")
    _check_cell_ptr(cell_ptr_next, n, "cell_ptr_next")
    max_pairs = _check_max_pairs(max_pairs)
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _mo._device_of(labels_prev, labels_next)
    a, b = _mo._to_device(labels_prev, dev), _mo._to_device(labels_next, dev)
    pa, pb = _mo._to_device(cell_ptr_prev, dev), _mo._to_device(cell_ptr_next, dev)
    if max_pairs is None:
        cells_prev, cells_next = (int(v) for v in torch.stack((pa[-1], pb[-1])).cpu().tolist())
        max_pairs = max(1, min(n * h * w, cells_prev * cells_next, MAX_PAIRS_LIMIT - 1))
    need = int(lib.rg_cell_overlap_workspace_bytes(max_pairs))
    if need < 0:
        _native.check(need, "rg_cell_overlap_workspace_bytes")
    with torch.cuda.device(dev):
        rows = torch.empty((max_pairs, 2), dtype=torch.int32, device=dev)
        count = torch.empty(max_pairs, dtype=torch.int32, device=dev)
        totals = torch.empty(2, dtype=torch.int32, device=dev)
        workspace = torch.empty(need // 8, dtype=torch.int64, device=dev)
        _native.check(lib.rg_cell_overlap_i32(_native.ptr(a), _native.ptr(pa), _native.ptr(b), _native.ptr(pb), n, h, w, max_pairs,
                                              _native.ptr(rows), _native.ptr(count), _native.ptr(totals), _native.ptr(workspace),
                                              need, _native.stream_ptr()), "rg_cell_overlap_i32")
        held, dropped = (int(v) for v in totals.cpu().tolist())                 # the one synchronisation
        if held > max_pairs or dropped:
            raise RuntimeError(f"cell_overlap_device: max_pairs = {max_pairs} is too small: the table holds {held} distinct "
                               f"pairs and {dropped} insertion(s) found it full")
        rows, count = rows[:held], count[:held]
        order = torch.sort((rows[:, 0].long() << 32) | rows[:, 1].long()).indices
        rows, count = rows[order], count[order]
    return CellOverlap(rows[:, 0].contiguous(), rows[:, 1].contiguous(), count.contiguous())


def relabel_cells_device(labels, cell_ptr, lut):
    """``lut[cell_ptr[p] + labels - 1]`` for every pixel of a cell, 0 elsewhere (``rg_relabel_cells_i32``): the plane of any
    per-cell int32 -- track ids, for display.  ``labels`` int32 ``[h, w]`` or ``[n, h, w]``, ``lut`` int32 ``[cells]``.  A
    label above its plane's cell count, or a row beyond ``lut``, gives 0.  No host synchronisation."""
    shape3 = _check_labels(labels, "labels")
    n, h, w = shape3
    _check_cell_ptr(cell_ptr, n, "cell_ptr")
    if not hasattr(lut, "shape") or _dtype_name(lut) != "int32" or len(lut.shape) != 1:
        raise ValueError("lut must be int32 [cells]")
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _mo._device_of(labels)
    src, ptr, table = _mo._to_device(labels, dev), _mo._to_device(cell_ptr, dev), _mo._to_device(lut, dev)
    with torch.cuda.device(dev):
        out = torch.empty(tuple(int(v) for v in labels.shape), dtype=torch.int32, device=dev)
        _native.check(lib.rg_relabel_cells_i32(_native.ptr(src), _native.ptr(ptr), n, h, w, _native.ptr(table), int(table.numel()),
                                               _native.ptr(out), _native.stream_ptr()), "rg_relabel_cells_i32")
    return out


# ---- host --------------------------------------------------------------------------------------------------------------------
def _best_partner(n: int, own, other, count) -> np.ndarray:
    """Per ``own`` row below ``n`` the ``other`` row with the largest count, ties to the smallest row; ``-1`` without a pair."""
    best = np.full(n, -1, dtype=np.int64)
    order = np.lexsort((other, -count.astype(np.int64), own))           # by own, then count descending, then other
    own, other = own[order], other[order]
    first = np.ones(len(own), dtype=bool)
    first[1:] = own[1:] != own[:-1]
    best[own[first]] = other[first]
    return best


def match_cells(overlap, area_prev, area_next, *, min_pixels: int = 1, min_fraction: float = 0.0) -> CellMatch:
    """Successor and predecessor of every cell from the overlap counts (host NumPy; integers but for one float64 comparison).

    ``overlap``: a :class:`CellOverlap` (device tensors or arrays); ``area_prev`` / ``area_next``: the ``area`` columns of the
    two cell tables, whose lengths are the cell counts.  A pair qualifies iff ``count >= min_pixels`` and ``count >=
    min_fraction * min(area_prev[a], area_next[b])``.  ``succ[a]`` is the qualifying partner of ``a`` with the largest count,
    ties to the smallest row, ``-1`` for none; ``pred[b]`` likewise."""
    min_pixels, min_fraction = _check_match_limits(min_pixels, min_fraction)
    try:
        row_prev, row_next, count = (_host(v) for v in overlap)
    except (TypeError, ValueError):
        raise ValueError("overlap must be a CellOverlap (row_prev, row_next, count)") from None
    area_prev, area_next = _host(area_prev), _host(area_next)
    if area_prev.ndim != 1 or area_next.ndim != 1 or not (row_prev.shape == row_next.shape == count.shape) or row_prev.ndim != 1:
        raise ValueError("overlap must hold three arrays of one length, the areas one row per cell")
    if len(row_prev) and (row_prev.min() < 0 or row_next.min() < 0 or row_prev.max() >= len(area_prev)
                          or row_next.max() >= len(area_next)):
        raise ValueError(f"overlap names rows beyond the {len(area_prev)} and {len(area_next)} cells of the two area columns")
    smaller = np.minimum(area_prev[row_prev], area_next[row_next])
    keep = (count >= min_pixels) & (count.astype(np.float64) >= min_fraction * smaller.astype(np.float64))
    a, b, c = row_prev[keep].astype(np.int64), row_next[keep].astype(np.int64), count[keep]
    return CellMatch(_best_partner(len(area_prev), a, b, c), _best_partner(len(area_next), b, a, c),
                     row_prev[keep], row_next[keep], c)


class TrackFrame(NamedTuple):
    """What :meth:`CellTracker.update` returns for one frame.  Device tensors first, then host arrays with one row per cell of
    ``table``."""
    labels: object           # int32 [h, w] on the device
    cell_ptr: object         # int32 [2] on the device
    table: object            # the frame's CellTable
    motion: object           # the filled MotionGrid (or the field given) the previous labels were moved along, or None
    track_id: np.ndarray     # int64: from 1, never reused
    parent_track: np.ndarray  # int64: the track this one split off from, 0 = none
    age: np.ndarray          # int64: frames since the track began, 0 for a new one
    velocity: np.ndarray     # float64 [n, 2] = (dy, dx) pixels per interval between the exact centroids; NaN for a new track
    ended: np.ndarray        # int64 [k, 2]: (track that ended with the previous frame, the track it merged into or 0)

    def track_plane_device(self):
        """int32 ``[h, w]`` on the device: every pixel's track id, 0 for background (``rg_relabel_cells_i32``)."""
        if len(self.track_id) and int(self.track_id.max()) > 2 ** 31 - 1:
            raise OverflowError(f"track id {int(self.track_id.max())} does not fit the int32 plane")
        return relabel_cells_device(self.labels, self.cell_ptr, self.track_id.astype(np.int32))


def assign_tracks(match: CellMatch, prev_track, prev_parent, prev_age, next_id: int):
    """The identity rules on the host.  ``prev_*``: the previous frame's per-cell ``track_id``, ``parent_track`` and ``age``;
    ``next_id``: the first unused track id.  Returns ``(track_id, parent_track, age, ended, next_id)``.

    Cells of the new frame, in row order: ``pred[b] == -1`` starts a track; ``succ[pred[b]] == b`` continues the track of
    ``pred[b]``; otherwise ``b`` starts a track whose parent is that of ``pred[b]`` (a split).  Cells of the old frame, in row
    order: ``succ[a] == -1`` ends the track; ``succ[a] == b`` with ``pred[b] != a`` ends it merged into ``b``'s track."""
    succ, pred = match.succ, match.pred
    n = len(pred)
    track, parent, age = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for b in range(n):
        a = int(pred[b])
        if a >= 0 and int(succ[a]) == b:
            track[b], parent[b], age[b] = prev_track[a], prev_parent[a], prev_age[a] + 1
        else:
            track[b], next_id = next_id, next_id + 1
            parent[b] = prev_track[a] if a >= 0 else 0
    ended = []
    for a in range(len(succ)):
        b = int(succ[a])
        if b < 0:
            ended.append((int(prev_track[a]), 0))
        elif int(pred[b]) != a:
            ended.append((int(prev_track[a]), int(track[b])))
    return track, parent, age, np.array(ended, dtype=np.int64).reshape(-1, 2), next_id


class CellTracker:
    """Storm cells with an identity that lasts: call :meth:`update` with every new product plane.

    ``threshold``, ``min_size``, ``connectivity``: what a cell is -- a connected region of ``plane >= threshold``; with
    ``min_size > 1`` the plane is despeckled first, so smaller regions never become cells.  ``min_pixels``, ``min_fraction``:
    when two cells count as the same (:func:`match_cells`).  ``motion``: how the previous frame's labels are brought to the
    new frame's time before they are compared -- ``"auto"`` estimates it between the two planes
    (:func:`~radar_processor_amd.motion.estimate_motion_device`, which takes ``**estimate_kw``, then
    :func:`~radar_processor_amd.motion.fill_motion_device`), ``None`` compares them where they are, a filled ``MotionGrid`` or
    a float32 ``[h, w, 2]`` field is used as given.  Without advection a cell that moves further than its own size per frame
    loses its track."""

    def __init__(self, threshold, *, min_size: int = 1, connectivity: int = 8, min_pixels: int = 1, min_fraction: float = 0.0,
                 motion="auto", **estimate_kw):
        lo = float(np.float32(threshold))
        if math.isnan(lo):
            raise ValueError(f"threshold must not be NaN, got {threshold!r}")
        if connectivity not in _cc.CONNECTIVITIES or isinstance(connectivity, bool):
            raise ValueError(f"connectivity must be 4 or 8, not {connectivity!r}")
        if not _is_int(min_size) or not 1 <= min_size < 2 ** 31:
            raise ValueError(f"min_size must be an integer of at least 1, not {min_size!r}")
        self.min_pixels, self.min_fraction = _check_match_limits(min_pixels, min_fraction)
        if isinstance(motion, str) and motion != "auto":
            raise ValueError(f"motion must be 'auto', None, a MotionGrid or a float32 [h, w, 2] field, not {motion!r}")
        unknown = sorted(set(estimate_kw) - set(_mo._ESTIMATE_KEYS))
        if unknown:
            raise ValueError(f"unknown keyword(s) {unknown}: expected some of {list(_mo._ESTIMATE_KEYS)}")
        if estimate_kw and not isinstance(motion, str):
            raise ValueError("estimation keywords only apply with motion='auto'")
        if estimate_kw:
            _mo._check_blocks(estimate_kw.get("block", 32), estimate_kw.get("stride", 16), estimate_kw.get("search", 16),
                              estimate_kw.get("min_echo"))
        self.threshold, self.min_size, self.connectivity = lo, int(min_size), int(connectivity)
        self.motion, self.estimate_kw = motion, dict(estimate_kw)
        self.next_id = 1
        self._prev = None                # (plane, TrackFrame, host area, host centroids) of the last frame

    def _move(self, labels, prev_plane, plane):
        """The previous labels at the new frame's time, and the motion used."""
        if self.motion is None:
            return labels, None
        if isinstance(self.motion, str):
            grid = _mo.fill_motion_device(_mo.estimate_motion_device(prev_plane, plane, **self.estimate_kw))
        else:
            grid = self.motion
        return advect_labels_device(labels, grid), grid

    def update(self, plane) -> TrackFrame:
        """Label ``plane`` (float32 ``[h, w]``, tensor or ndarray), match its cells to the previous frame's and return the
        :class:`TrackFrame`.  Synchronises with the host: the cell count, the overlap's ``totals`` and the per-cell areas and
        index sums come back every frame."""
        if _cc._check_planes(plane, "plane")[0] != 1 or len(plane.shape) != 2:
            raise ValueError(f"plane must be one float32 [h, w] plane, got {list(plane.shape)}")
        if self._prev is not None and tuple(self._prev[0].shape) != tuple(int(v) for v in plane.shape):
            raise ValueError(f"plane of shape {list(plane.shape)} after frames of shape {list(self._prev[0].shape)}")
        dev = _cc._device_of(plane)
        plane = _cc._to_device(plane, dev)
        cells_of = plane
        if self.min_size > 1:
            cells_of = _cc.despeckle_device(plane, self.threshold, self.min_size, connectivity=self.connectivity)
        labels, cell_ptr = _cc.label_components_device(cells_of, self.threshold, connectivity=self.connectivity)
        table = _cc.cell_table_device(cells_of, labels, cell_ptr)
        area = _host(table.area).astype(np.int64)
        centroid = _host(table.sum_yx).astype(np.float64) / area[:, None].astype(np.float64)
        n = len(area)
        velocity = np.full((n, 2), np.nan, dtype=np.float64)
        if self._prev is None:
            track = np.arange(self.next_id, self.next_id + n, dtype=np.int64)
            parent, age, ended, grid = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros((0, 2), np.int64), None
            self.next_id += n
        else:
            prev_plane, prev, prev_area, prev_centroid = self._prev
            moved, grid = self._move(prev.labels, prev_plane, plane)
            overlap = cell_overlap_device(moved, prev.cell_ptr, labels, cell_ptr)
            match = match_cells(overlap, prev_area, area, min_pixels=self.min_pixels, min_fraction=self.min_fraction)
            track, parent, age, ended, self.next_id = assign_tracks(match, prev.track_id, prev.parent_track, prev.age, self.next_id)
            kept = age > 0
            velocity[kept] = centroid[kept] - prev_centroid[match.pred[kept]]
        frame = TrackFrame(labels, cell_ptr, table, grid, track, parent, age, velocity, ended)
        self._prev = (plane, frame, area, centroid)
        return frame
