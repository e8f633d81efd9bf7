"""Doppler velocity dealiasing by regions, on the device (include/radargrid_velocity.h; kernels in csrc/rg_velocity.hip): what a
volume's radial velocity needs BEFORE it is gridded.  A wind faster than the Nyquist velocity ``Vn`` folds back into
``[-Vn, +Vn]``, and a gridder's weighted mean averages ``+Vn`` with ``-Vn`` across the fold line into a calm that is not there.

The algorithm is the region-based one (PyART's ``dealias_region_based``), restated in integers:

* :func:`split_velocity_device` splits ``[-Vn, Vn]`` into bands (``rg_velocity_split_f32``);
* :func:`velocity_regions_device` labels the connected regions of every band with the labeller of :mod:`components` and gives
  every gate one global region id (``rg_velocity_regions_i32``);
* :func:`region_edges_device` builds the region adjacency table: per pair of touching regions the gate pairs they share and the
  exact sum of the velocity differences across the border, in 2^-16 m/s fixed point (``rg_region_edges_f32``);
* :func:`merge_regions` merges the regions greedily by the strongest edge and unfolds the smaller side by whole Nyquist
  intervals: host code, pure integers, no device;
* :func:`apply_folds_device` adds each region's fold (``rg_velocity_apply_folds_f32``);
* :func:`dealias_velocity_device` chains them; :func:`dealias_velocity` is its NumPy-in, NumPy-out form.

A volume is float32 ``[n_sweeps, n_rays, n_gates]`` (tensor or ndarray); a 2-D input is one sweep.  ``nyquist`` is one number or
one per sweep.  The dealiased ``velocity.reshape(-1)`` is what ``fields`` of the gridders take.

The limit of the method: an echo island that touches no other region cannot be tied to the rest of the sweep, so every
connected set of regions is centred on its own most common fold.  Anchoring to a sounding or to the sweep below, bridging gaps
between rays or gates and dual-PRF outliers are out of scope.

The contract is this build's own (the header states it; ``tests/velocity_oracle.py`` restates it in NumPy and the tests hold the
kernels EQUAL to that, bit for bit: every sum is an integer).  Parity with PyART is unpinned.  The device functions enqueue on
torch's current stream and validate every argument before the device is touched.
"""
from __future__ import annotations

import heapq
import math
from typing import NamedTuple, Optional, Tuple

import numpy as np

from . import _native
from . import components as _cc
from .motion import _device_of, _dtype_name, _is_int, _to_device

MAX_ABS = _native.RG_VELOCITY_MAX_ABS
MAX_NYQUIST = _native.RG_VELOCITY_MAX_NYQUIST
MIN_BANDS = _native.RG_VELOCITY_MIN_BANDS
MAX_BANDS = _native.RG_VELOCITY_MAX_BANDS
MAX_EDGES_LIMIT = 2 ** 30            # rg_region_edges_f32 takes 1 <= max_edges < 2^30
_FLT_MAX = float(np.finfo(np.float32).max)


class VelocityRegions(NamedTuple):
    """What :func:`velocity_regions_device` returns: ``regions`` int32 of the volume's shape on the device (0 = no region, ids
    from 1 = row of the cell table + 1), ``n_regions``, ``sizes`` int32 ``[n_regions]`` on the device (gates per region) and
    ``cell_ptr`` int32 ``[n_sweeps * n_bands + 1]`` on the device (region row ``k`` lies in plane ``p`` with ``cell_ptr[p] <= k
    < cell_ptr[p + 1]``, and its sweep is ``p // n_bands``)."""
    regions: object
    n_regions: int
    sizes: object
    cell_ptr: object


class RegionEdges(NamedTuple):
    """What :func:`region_edges_device` returns, sorted by ``(lo, hi)``: ``pairs`` int32 ``[n, 2]``, ``count`` int32 ``[n]``
    and ``sum`` int64 ``[n]`` on the device, and ``totals`` = (edges the table holds, insertions that found it full) on the
    host.  The table is complete iff ``totals[0] == n and totals[1] == 0``."""
    pairs: object
    count: object
    sum: object
    totals: Tuple[int, int]


class DealiasedVelocity(NamedTuple):
    """What :func:`dealias_velocity_device` returns: ``velocity`` float32 (NaN where a gate is not valid), ``folds`` int32 (the
    Nyquist intervals added; 0 where ``velocity`` is NaN) and ``regions`` int32, each of the input's shape, then the number of
    regions and of edges between them."""
    velocity: object
    folds: object
    regions: object
    n_regions: int
    n_edges: int


# ---- validation (host only) --------------------------------------------------------------------------------------------------
def _check_volume(vel, what: str, dtype: str = "float32") -> Tuple[int, int, int]:
    """``(S, R, G)`` of ``[R, G]`` or ``[S, R, G]`` (tensor or ndarray), by dtype and rank only."""
    if not hasattr(vel, "shape") or not hasattr(vel, "dtype"):
        raise ValueError(f"{what} must be a tensor or an ndarray, not {type(vel).__name__}")
    shape = tuple(int(n) for n in vel.shape)
    if _dtype_name(vel) != dtype or len(shape) not in (2, 3):
        raise ValueError(f"{what} must be {dtype} [n_rays, n_gates] or [n_sweeps, n_rays, n_gates]; got {_dtype_name(vel)} "
                         f"{list(shape)}")
    shape3 = (1,) + shape if len(shape) == 2 else shape
    if shape3[0] < 1 or shape3[1] < 1:
        raise ValueError(f"{what}: at least one sweep and one ray; got {list(shape)}")
    return shape3


def _check_bands(n_bands, shape3) -> int:
    if not _is_int(n_bands) or not MIN_BANDS <= n_bands <= MAX_BANDS:
        raise ValueError(f"n_bands must be an integer in {MIN_BANDS} .. {MAX_BANDS}, not {n_bands!r}")
    if shape3[0] * shape3[1] * shape3[2] * int(n_bands) >= 2 ** 31:
        raise ValueError(f"{list(shape3)} gates in {n_bands} bands are 2^31 or more: split the volume by sweeps")
    return int(n_bands)


def _check_nyquist(nyquist, n_sweeps: int):
    """The ctypes ``double [n_sweeps]`` the library takes: one number for all sweeps, or one per sweep."""
    try:
        values = np.asarray(nyquist.detach().cpu().numpy() if hasattr(nyquist, "detach") else nyquist, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"nyquist must be a number or one number per sweep, not {nyquist!r}") from None
    if values.ndim == 0:
        values = np.full(n_sweeps, float(values))
    if values.shape != (n_sweeps,):
        raise ValueError(f"nyquist: one number, or one per sweep ({n_sweeps}); got shape {list(values.shape)}")
    for v in values.tolist():
        if not (math.isfinite(v) and 0.0 < v <= MAX_NYQUIST) or interval_of(v) < 1:
            raise ValueError(f"nyquist must be finite with 0 < Vn <= {MAX_NYQUIST} (and at least 2^-17), got {v!r}")
    return (_native.c_double * n_sweeps)(*values.tolist())


def _check_like(other, vel, what: str, dtype: Optional[str]) -> None:
    """``other`` (optional) has the shape of ``vel`` and, unless ``dtype`` is None, that dtype."""
    if other is None:
        return
    if not hasattr(other, "shape") or tuple(int(n) for n in other.shape) != tuple(int(n) for n in vel.shape):
        raise ValueError(f"{what} of shape {list(getattr(other, 'shape', []))} for a volume of shape {list(vel.shape)}")
    if dtype is not None and _dtype_name(other) != dtype:
        raise ValueError(f"{what} must be {dtype}, got {_dtype_name(other)}")


def _check_max_edges(max_edges) -> Optional[int]:
    if max_edges is None:
        return None
    if not _is_int(max_edges) or not 1 <= max_edges < MAX_EDGES_LIMIT:
        raise ValueError(f"max_edges must be an integer in 1 .. 2^30 - 1 or None, not {max_edges!r}")
    return int(max_edges)


def interval_of(nyquist: float) -> int:
    """The Nyquist interval ``2 * Vn`` in the fixed point of the edge sums: ``llrint(65536 * 2.0 * Vn)``."""
    return int(np.rint(65536.0 * 2.0 * float(nyquist)))


def default_max_edges(n_regions: int) -> int:
    """``max(3 * n_regions, 64)``: the region adjacency graph is a contraction of a planar grid graph (a cylinder with
    ``wrap_rows`` is planar too), so ``n >= 3`` regions have at most ``3 n - 6`` edges."""
    return max(3 * int(n_regions), 64)


# ---- device ------------------------------------------------------------------------------------------------------------------
def _split(lib, torch, src, m, shape3, nyq, n_bands):
    S, R, G = shape3
    split = torch.empty((S, n_bands, R, G), dtype=torch.float32, device=src.device)
    if G:                        # rays without gates: the empty output is the result (and an empty tensor has no address)
        _native.check(lib.rg_velocity_split_f32(_native.ptr(src), _native.ptr(m), S, R, G, nyq, n_bands, _native.ptr(split),
                                                _native.stream_ptr()), "rg_velocity_split_f32")
    return split


def _regions(lib, torch, src, m, shape3, nyq, n_bands, wrap_rays, timings=None) -> VelocityRegions:
    """split -> label -> (the one read of the region count) -> areas -> flatten."""
    S, R, G = shape3
    dev = src.device
    if G == 0:
        return VelocityRegions(torch.zeros(shape3, dtype=torch.int32, device=dev), 0, torch.zeros(0, dtype=torch.int32, device=dev),
                               torch.zeros(S * n_bands + 1, dtype=torch.int32, device=dev))
    split = _split(lib, torch, src, m, shape3, nyq, n_bands)
    stack = (S * n_bands, R, G)
    labels, cell_ptr = _cc._label(lib, torch, split, None, stack, -_FLT_MAX, float("inf"), 4, wrap_rays)
    n_regions = int(cell_ptr[-1].item())                       # the one synchronisation
    sizes = torch.empty(n_regions, dtype=torch.int32, device=dev)
    _native.check(lib.rg_component_stats_f32(_native.ptr(split), _native.ptr(labels), _native.ptr(cell_ptr), *stack, n_regions,
                                             _native.ptr(sizes), 0, 0, 0, 0, 0, _native.stream_ptr()), "rg_component_stats_f32")
    regions = torch.empty(shape3, dtype=torch.int32, device=dev)
    _native.check(lib.rg_velocity_regions_i32(_native.ptr(labels), _native.ptr(cell_ptr), S, R, G, n_bands, _native.ptr(regions),
                                              _native.stream_ptr()), "rg_velocity_regions_i32")
    return VelocityRegions(regions, n_regions, sizes, cell_ptr)


def _edges(lib, torch, values, regions, shape3, wrap_rows, max_edges) -> RegionEdges:
    n, h, w = shape3
    dev = values.device
    if h == 0 or w == 0:         # no pixels: the empty table is the result (and an empty tensor has no address)
        return RegionEdges(torch.zeros((0, 2), dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                           torch.zeros(0, dtype=torch.int64, device=dev), (0, 0))
    need = int(lib.rg_region_edges_workspace_bytes(max_edges))
    if need < 0:
        _native.check(need, "rg_region_edges_workspace_bytes")
    pairs = torch.empty((max_edges, 2), dtype=torch.int32, device=dev)
    count = torch.empty(max_edges, dtype=torch.int32, device=dev)
    total = torch.empty(max_edges, dtype=torch.int64, device=dev)
    totals = torch.empty(2, dtype=torch.int32, device=dev)
    workspace = torch.empty(need // 8, dtype=torch.int64, device=dev)
    _native.check(lib.rg_region_edges_f32(_native.ptr(values), _native.ptr(regions), n, h, w, 1 if wrap_rows else 0, max_edges,
                                          _native.ptr(pairs), _native.ptr(count), _native.ptr(total), _native.ptr(totals),
                                          _native.ptr(workspace), need, _native.stream_ptr()), "rg_region_edges_f32")
    held, dropped = (int(v) for v in totals.cpu().tolist())    # the one synchronisation
    kept = min(held, max_edges)
    pairs, count, total = pairs[:kept], count[:kept], total[:kept]
    order = torch.sort((pairs[:, 0].long() << 32) | pairs[:, 1].long()).indices
    return RegionEdges(pairs[order].contiguous(), count[order].contiguous(), total[order].contiguous(), (held, dropped))


def _apply(lib, torch, src, regions, lut, shape3, nyq, want_folds):
    S, R, G = shape3
    out = torch.empty(shape3, dtype=torch.float32, device=src.device)
    folds = torch.empty(shape3, dtype=torch.int32, device=src.device) if want_folds else None
    if G:
        _native.check(lib.rg_velocity_apply_folds_f32(_native.ptr(src), _native.ptr(regions), _native.ptr(lut) if lut.numel() else 0,
                                                      int(lut.numel()), S, R, G, nyq, _native.ptr(out), _native.ptr(folds),
                                                      _native.stream_ptr()), "rg_velocity_apply_folds_f32")
    return out, folds


def split_velocity_device(vel, nyquist, *, n_bands: int = 3, mask=None):
    """The volume split into its velocity bands: float32 ``[n_sweeps, n_bands, n_rays, n_gates]`` on the device (``[n_bands,
    n_rays, n_gates]`` for a 2-D input).  Plane ``(s, b)`` holds ``v`` where the gate is valid -- finite, ``|v| <= 16384`` and
    ``mask`` (optional, any integer or bool type; non-zero leaves the gate out) zero -- and its band
    ``clamp(floor((v + Vn) * n_bands / (2 Vn)), 0, n_bands - 1)`` is ``b``; NaN elsewhere.  No host synchronisation."""
    shape3 = _check_volume(vel, "vel")
    n_bands = _check_bands(n_bands, shape3)
    nyq = _check_nyquist(nyquist, shape3[0])
    _check_like(mask, vel, "mask", None)
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(vel, mask)
    src = _to_device(vel, dev)
    m = None if mask is None else _to_device(mask, dev, torch.uint8)
    with torch.cuda.device(dev):
        split = _split(lib, torch, src, m, shape3, nyq, n_bands)
    return split[0] if len(vel.shape) == 2 else split


def velocity_regions_device(vel, nyquist, *, n_bands: int = 3, mask=None, wrap_rays: bool = True) -> VelocityRegions:
    """The regions of a volume: the 4-connected sets of valid gates of one band within one sweep; with ``wrap_rays`` the first
    and the last ray of a sweep are neighbours (a full PPI).  Regions are numbered from 1 by sweep, band and the raster order of
    their first gate.  Reads the region count once -- its one host synchronisation.  Returns :class:`VelocityRegions`."""
    shape3 = _check_volume(vel, "vel")
    n_bands = _check_bands(n_bands, shape3)
    nyq = _check_nyquist(nyquist, shape3[0])
    _check_like(mask, vel, "mask", None)
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(vel, mask)
    src = _to_device(vel, dev)
    m = None if mask is None else _to_device(mask, dev, torch.uint8)
    with torch.cuda.device(dev):
        got = _regions(lib, torch, src, m, shape3, nyq, n_bands, wrap_rays)
    return got._replace(regions=got.regions.reshape(tuple(vel.shape)))


def region_edges_device(values, regions, *, wrap_rows: bool, max_edges: Optional[int] = None) -> RegionEdges:
    """The region adjacency table of ``regions`` (int32, 0 = none) over ``values`` (float32), both ``[h, w]`` or ``[n, h, w]``:
    for every pair of regions ``lo < hi`` that touch -- horizontally, vertically and, with ``wrap_rows`` and ``h >= 3``, across
    the seam between the last and the first row -- the pixel pairs they share and the sum of ``q(hi pixel) - q(lo pixel)`` with
    ``q = llrint(65536 * value)``.  A pair counts when both values are finite and at most 16384 in magnitude.  Planes never pair.

    ``max_edges`` sizes the hash table (twice that many slots) and the outputs.  ``None``: ``max(3 * regions.max(), 64)``,
    which suffices for regions that are connected sets (a planar graph) and costs one read of the largest id.  The function
    reads ``totals`` once -- its host synchronisation -- and does NOT raise on an incomplete table: compare ``totals`` with the
    rows returned.  Returns :class:`RegionEdges`, sorted by ``(lo, hi)``."""
    shape3 = _check_volume(values, "values")
    if _check_volume(regions, "regions", "int32") != shape3 or tuple(values.shape) != tuple(regions.shape):
        raise ValueError(f"values of shape {list(values.shape)} and regions of shape {list(regions.shape)} differ")
    if shape3[0] * shape3[1] * shape3[2] >= 2 ** 31:
        raise ValueError(f"values: {list(values.shape)} holds 2^31 pixels or more")
    max_edges = _check_max_edges(max_edges)
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(values, regions)
    v, r = _to_device(values, dev), _to_device(regions, dev)
    with torch.cuda.device(dev):
        if max_edges is None:
            max_edges = min(default_max_edges(max(int(r.max().item()), 0) if r.numel() else 0), MAX_EDGES_LIMIT - 1)
        return _edges(lib, torch, v, r, shape3, wrap_rows, max_edges)


def apply_folds_device(vel, regions, fold_lut, nyquist, *, return_folds: bool = False):
    """``vel + fold_lut[regions - 1] * 2 Vn`` in float64, rounded once to float32, of the volume's shape on the device; NaN
    where ``regions`` is 0 or above ``len(fold_lut)``.  ``return_folds=True`` also returns the int32 fold per gate (0 where the
    result is NaN).  No host synchronisation."""
    shape3 = _check_volume(vel, "vel")
    _check_like(regions, vel, "regions", "int32")
    if regions is None:
        raise ValueError("regions is required")
    if not hasattr(fold_lut, "shape") or _dtype_name(fold_lut) != "int32" or len(fold_lut.shape) != 1:
        raise ValueError("fold_lut must be int32 [n_regions]")
    if shape3[0] * shape3[1] * shape3[2] >= 2 ** 31:
        raise ValueError(f"vel: {list(vel.shape)} holds 2^31 gates or more")
    nyq = _check_nyquist(nyquist, shape3[0])
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(vel, regions)
    src, r, lut = _to_device(vel, dev), _to_device(regions, dev), _to_device(fold_lut, dev)
    with torch.cuda.device(dev):
        out, folds = _apply(lib, torch, src, r, lut, shape3, nyq, return_folds)
    out = out.reshape(tuple(vel.shape))
    return (out, folds.reshape(tuple(vel.shape))) if return_folds else out


# ---- host --------------------------------------------------------------------------------------------------------------------
def merge_regions(edges, sizes, interval_of_region) -> np.ndarray:
    """The fold of every region, int64 ``[n_regions]``: pure integers, deterministic, no device.

    ``edges``: rows ``(lo, hi, count, sum)`` with 1-based region ids ``lo < hi``, ``sum`` the sum of ``q(hi) - q(lo)`` over the
    ``count`` gate pairs of the border (:func:`region_edges_device`); ``sizes[k]``: the gates of region ``k + 1``;
    ``interval_of_region[k]``: the Nyquist interval of its sweep in the same fixed point (:func:`interval_of`).

    Sets start as single regions with fold 0; a set is named by the smallest region id it contains.  An edge between the sets
    X and Y carries ``(C, S)``, ``S`` oriented Y - X.  Until no edge is left: take the edge with the largest ``C`` (ties: the
    smallest ``(lo, hi)`` of the current set names).  The base is the set with more gates (a tie: the smaller name), the other
    set M is merged into it: with ``S`` oriented M - base and ``W = C * I`` (``I`` the interval of M; edges never join two
    sweeps), ``n = (2 S + W) // (2 W)`` -- the nearest whole number of intervals, a half rounding up -- and every region of M
    gets ``fold -= n``.  Every other edge of M, oriented X - M, gets ``S += n * C_x * I`` and is added, count and sum, into the
    base's edge to X.  Sets that never touch stay independent.  Last, per set, the fold held by the most gates becomes 0 (ties:
    the smallest ``|fold|``, then the negative one).

    The strongest edge comes from a heap with lazy deletion, the folds of a merged set are shifted through a union-find with
    offsets: about ``(edges + regions) * log`` steps in all."""
    sizes = [int(v) for v in np.asarray(sizes).reshape(-1).tolist()]
    n = len(sizes)
    intervals = [int(v) for v in np.asarray(interval_of_region).reshape(-1).tolist()]
    if len(intervals) != n:
        raise ValueError(f"interval_of_region holds {len(intervals)} entries for {n} regions")
    if any(v < 1 for v in intervals):
        raise ValueError("interval_of_region: every interval must be at least 1")
    rows = np.asarray(edges, dtype=object).reshape(-1, 4).tolist() if len(edges) else []
    # adj[X][Y] = [C, S], S oriented Y - X; both directions are kept.  Sets are keyed by name (0-based region index here).
    adj = {}
    for lo, hi, c, s in rows:
        lo, hi, c, s = int(lo) - 1, int(hi) - 1, int(c), int(s)
        if not (0 <= lo < hi < n) or c < 1:
            raise ValueError(f"edge ({lo + 1}, {hi + 1}, {c}, {s}): ids must satisfy 1 <= lo < hi <= {n} and count >= 1")
        if hi in adj.setdefault(lo, {}):
            raise ValueError(f"edge ({lo + 1}, {hi + 1}) appears twice")
        adj[lo][hi] = [c, s]
        adj.setdefault(hi, {})[lo] = [c, -s]
    heap = [(-cs[0], x, y) for x, nb in adj.items() for y, cs in nb.items() if x < y]
    heapq.heapify(heap)
    gates = dict(enumerate(sizes))                 # set name -> gates, for the sets that still exist
    parent = list(range(n))                        # union-find with offsets: fold(r) = fold(parent[r]) + shift[r]
    shift = [0] * n
    root = list(range(n))                          # set name -> the root of its tree (the name itself need not be the root)

    while heap:
        neg_c, lo, hi = heapq.heappop(heap)
        edge = adj.get(lo)
        if edge is not None:
            edge = edge.get(hi)
        if edge is None or edge[0] != -neg_c:
            continue                               # an entry of an edge that has merged or grown since
        base, m = (lo, hi) if gates[lo] >= gates[hi] else (hi, lo)
        c, s = adj[base][m]                        # oriented M - base
        w = c * intervals[m]
        k = (2 * s + w) // (2 * w)
        name = lo                                  # the merged set keeps the smaller name
        parent[root[m]] = root[base]               # every region of M: fold -= k; the base's regions never move
        shift[root[m]] = -k
        root[name] = root[base]
        merged = adj.pop(base)
        del merged[m]
        touched = []                               # the neighbours whose edge to the merged set is new or has grown
        for x, (cx, sx) in adj.pop(m).items():
            if x == base:
                continue
            sx += k * cx * intervals[m]
            if x in merged:
                merged[x][0] += cx
                merged[x][1] += sx
            else:
                merged[x] = [cx, sx]
            del adj[x][m]
            touched.append(x)
        gates[name] = gates.pop(base) + gates.pop(m)
        adj[name] = merged
        if name != base:                           # renamed: every neighbour knows the set by its old name
            for x in merged:
                adj[x].pop(base, None)
            touched = list(merged)
        for x in touched:
            cx, sx = merged[x]
            adj[x][name] = [cx, -sx]
            heapq.heappush(heap, (-cx, name, x) if name < x else (-cx, x, name))

    def find(r):
        path = []
        while parent[r] != r:
            path.append(r)
            r = parent[r]
        total = 0
        for q in reversed(path):                   # from the root down: every node of the path ends up a child of the root
            total += shift[q]
            shift[q] = total
            parent[q] = r
        return r

    folds = np.zeros(n, dtype=np.int64)
    members = {}
    for r in range(n):
        root = find(r)
        folds[r] = shift[r] if r != root else 0
        members.setdefault(root, []).append(r)
    for regs in members.values():
        weight = {}
        for r in regs:
            weight[int(folds[r])] = weight.get(int(folds[r]), 0) + sizes[r]
        centre = min(weight, key=lambda f: (-weight[f], abs(f), f))
        if centre:
            folds[regs] -= centre
    return folds


def region_intervals(cell_ptr, nyquist, n_bands: int) -> np.ndarray:
    """``interval_of_region`` for :func:`merge_regions`: int64 ``[n_regions]`` from the host copy of ``cell_ptr`` and the
    Nyquist velocity of every sweep."""
    cell_ptr = np.asarray(cell_ptr, dtype=np.int64)
    per_plane = np.repeat(np.array([interval_of(v) for v in nyquist], dtype=np.int64), n_bands)
    return np.repeat(per_plane, np.diff(cell_ptr))


def dealias_velocity_device(vel, nyquist, *, n_bands: int = 3, mask=None, wrap_rays: bool = True, timings: Optional[dict] = None
                            ) -> DealiasedVelocity:
    """The chain on one volume: split ``vel`` into ``n_bands`` bands, label their regions, build the adjacency table, merge
    on the host, add the folds.  ``vel`` float32 ``[n_sweeps, n_rays, n_gates]`` or ``[n_rays, n_gates]`` (one sweep);
    ``nyquist`` one number or one per sweep; ``mask`` non-zero leaves a gate out; ``wrap_rays``: every sweep is a full circle.

    The chain synchronises with the host TWICE, by its nature: once for the number of regions (it sizes the table), once for
    the edges (the merge is host code).  The table is sized ``max(3 * n_regions, 64)``; the region graph is planar, so it has at
    most ``3 n - 6`` edges and an incomplete table is a bug: ``RuntimeError``.

    ``timings`` (optional dict) receives ``merge_ms``, the host milliseconds of the merge.  Returns :class:`DealiasedVelocity`."""
    shape3 = _check_volume(vel, "vel")
    n_bands = _check_bands(n_bands, shape3)
    nyq = _check_nyquist(nyquist, shape3[0])
    _check_like(mask, vel, "mask", None)
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(vel, mask)
    src = _to_device(vel, dev)
    m = None if mask is None else _to_device(mask, dev, torch.uint8)
    with torch.cuda.device(dev):
        reg = _regions(lib, torch, src, m, shape3, nyq, n_bands, wrap_rays)             # synchronisation 1: the region count
        n_edges = 0
        if reg.n_regions:
            max_edges = min(default_max_edges(reg.n_regions), MAX_EDGES_LIMIT - 1)
            edges = _edges(lib, torch, src, reg.regions, shape3, wrap_rays, max_edges)   # synchronisation 2: the edges
            held, dropped = edges.totals
            if held > max_edges or dropped:
                raise RuntimeError(f"dealias_velocity_device: {reg.n_regions} regions gave {held} edges ({dropped} dropped), more "
                                   f"than the planar bound the table of {max_edges} was sized by")
            n_edges = held
            host = torch.cat((edges.pairs.long(), edges.count.long()[:, None], edges.sum[:, None]), dim=1).cpu().numpy()
            sizes, cell_ptr = reg.sizes.cpu().numpy(), reg.cell_ptr.cpu().numpy()
            import time
            t0 = time.perf_counter()
            lut = merge_regions(host, sizes, region_intervals(cell_ptr, list(nyq), n_bands))
            if timings is not None:
                timings["merge_ms"] = (time.perf_counter() - t0) * 1e3
            lut = torch.from_numpy(lut.astype(np.int32)).to(dev)
        else:
            lut = torch.zeros(0, dtype=torch.int32, device=dev)
        out, folds = _apply(lib, torch, src, reg.regions, lut, shape3, nyq, True)
    shape = tuple(vel.shape)
    return DealiasedVelocity(out.reshape(shape), folds.reshape(shape), reg.regions.reshape(shape), reg.n_regions, n_edges)


def dealias_velocity(vel, nyquist, **kw) -> DealiasedVelocity:
    """:func:`dealias_velocity_device` for NumPy arrays: the volume is staged through device memory and ``velocity``, ``folds``
    and ``regions`` come back as ndarrays."""
    r = dealias_velocity_device(vel, nyquist, **kw)
    return DealiasedVelocity(r.velocity.cpu().numpy(), r.folds.cpu().numpy(), r.regions.cpu().numpy(), r.n_regions, r.n_edges)
