"""Echo motion and nowcasts on the device (include/radargrid_hip.h, "Echo motion and nowcasts"; kernels in
csrc/rg_motion.hip): where the echo is going, and the product plane 5 to 60 minutes ahead.

* :func:`quantize_planes_device` turns float32 planes into 8-bit levels (0 = no echo);
* :func:`estimate_motion_device` finds one motion vector per block of ``prev`` by exhaustive normalised cross-correlation
  in ``next`` (``rg_block_match_u8``) and returns a :class:`MotionGrid`;
* :func:`fill_motion_device` replaces the vectors that are missing or poorly correlated;
* :func:`advect_device` extrapolates planes along a motion field (``rg_advect_f32``, semi-Lagrangian, backward);
* :func:`nowcast_device` chains the four, :func:`nowcast` is its NumPy-in, NumPy-out wrapper;
* :func:`motion_to_velocity` converts pixels per interval into metres per second on a grid (host).

SIGN AND UNITS: echo at pixel ``p`` of ``prev`` is found at ``p + motion`` in ``next``; a vector is ``(dy, dx)`` in pixels per
interval between the two planes; the row index grows northwards, as in every grid here.

The device functions take tensors or ndarrays, enqueue on torch's current stream, validate every argument before the device
is touched and never synchronise with the host.  The kernels are pinned bit for bit to the NumPy restatement of the header's
formulas (``tests/motion_oracle.py``).
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import numpy as np

from . import _native

ADVECT_METHODS = {"nearest": 0, "bilinear": 1}
MAX_BLOCK = _native.RG_MOTION_MAX_BLOCK
MAX_SEARCH = _native.RG_MOTION_MAX_SEARCH
MAX_LEADS = _native.RG_MAX_LEADS
MAX_SUBSTEPS = 16
_ESTIMATE_KEYS = ("block", "stride", "search", "lo", "hi", "min_echo", "mask_prev", "mask_next")
_ADVECT_KEYS = ("method", "substeps", "fill_value", "out")


class Lattice(NamedTuple):
    """Field for field the ``rg_motion_lattice``: node ``(j, i)`` of a motion field lies at pixel
    ``(origin_y + j * step_y, origin_x + i * step_x)``."""
    origin_y: float
    origin_x: float
    step_y: float
    step_x: float
    ny: int
    nx: int


class MotionGrid(NamedTuple):
    """What :func:`estimate_motion_device` returns.  ``motion`` float32 ``[.., nby, nbx, 2]`` = ``(dy, dx)`` with the
    sub-pixel offset, ``score`` float32 ``[.., nby, nbx]`` the winning correlation, ``disp`` int16 ``[.., nby, nbx, 2]`` the
    integer winner; a block without enough echo, without contrast or without a candidate holds NaN (``disp`` 0).  The
    leading axis is there when the planes had one.  Node ``(j, i)`` sits at pixel ``origin + (j, i) * step`` of a plane of
    ``shape``: ``origin = (block - 1) / 2``, the block's centre, and ``step = stride``."""
    motion: object
    score: object
    disp: object
    block: int
    stride: int
    search: int
    shape: Tuple[int, int]
    origin: float
    step: float

    @property
    def lattice(self) -> Lattice:
        ny, nx = (int(v) for v in self.motion.shape[-3:-1])
        return Lattice(self.origin, self.origin, self.step, self.step, ny, nx)


def block_lattice(shape, block: int, stride: int) -> Lattice:
    """The lattice of block centres of a plane ``(h, w)``: ``(h - block) // stride + 1`` rows of nodes from
    ``(block - 1) / 2`` every ``stride`` pixels, likewise columns.  ``ValueError`` when the plane is smaller than a block."""
    h, w = (int(v) for v in tuple(shape)[-2:])
    block, stride, _, _ = _check_blocks(block, stride, 0)
    if h < block or w < block:
        raise ValueError(f"planes of {[h, w]} are smaller than a block of {block}")
    origin = (block - 1) / 2.0
    return Lattice(origin, origin, float(stride), float(stride), (h - block) // stride + 1, (w - block) // stride + 1)


# ---- validation (host only) --------------------------------------------------------------------------------------------------
def _is_tensor(a) -> bool:
    return type(a).__module__.startswith("torch")


def _dtype_name(a) -> str:
    return str(a.dtype).replace("torch.", "")


def _is_int(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def _check_planes(planes, what: str, dtypes=("float32",)):
    """``(n, h, w)`` of ``[h, w]`` or ``[n, h, w]`` planes (tensor or ndarray), by dtype and rank only."""
    if not hasattr(planes, "shape") or not hasattr(planes, "dtype"):
        raise ValueError(f"{what} must be a tensor or an ndarray, not {type(planes).__name__}")
    shape = tuple(int(n) for n in planes.shape)
    if _dtype_name(planes) not in dtypes or len(shape) not in (2, 3):
        raise ValueError(f"{what} must be {' or '.join(dtypes)} [h, w] or [n, h, w]; got {_dtype_name(planes)} {list(shape)}")
    shape3 = (1,) + shape if len(shape) == 2 else shape
    if shape3[0] < 1:
        raise ValueError(f"{what}: no planes in shape {list(shape)}")
    if shape3[0] * shape3[1] * shape3[2] >= 2 ** 31:
        raise ValueError(f"{what}: {list(shape)} holds 2^31 pixels or more")
    return shape3


def _check_levels(lo, hi) -> Tuple[float, float]:
    """``(lo, inv_step)`` as the float32 values the kernel takes; ``inv_step = float32(254 / (hi - lo))`` from doubles."""
    lo, hi = float(lo), float(hi)
    if not (math.isfinite(lo) and math.isfinite(hi)) or not hi > lo:
        raise ValueError(f"lo and hi must be finite with hi > lo, got {lo!r} and {hi!r}")
    with np.errstate(over="ignore"):
        lo32, inv = float(np.float32(lo)), float(np.float32(254.0 / (hi - lo)))
    if not (math.isfinite(lo32) and math.isfinite(inv) and inv > 0.0):
        raise ValueError(f"lo {lo!r} and hi {hi!r} leave no float32 level step")
    return lo32, inv


def _check_mask(mask, planes, what: str) -> None:
    if mask is not None and (not hasattr(mask, "shape") or tuple(int(n) for n in mask.shape) !=
                             tuple(int(n) for n in planes.shape)):
        raise ValueError(f"{what} of shape {list(getattr(mask, 'shape', []))} for planes of shape {list(planes.shape)}")


def _check_blocks(block, stride, search, min_echo=None):
    if not _is_int(block) or not 4 <= block <= MAX_BLOCK or block % 4:
        raise ValueError(f"block must be a multiple of 4 in 4 .. {MAX_BLOCK}, not {block!r}")
    if not _is_int(stride) or not 1 <= stride < 2 ** 31:
        raise ValueError(f"stride must be an integer of at least 1, not {stride!r}")
    if not _is_int(search) or not 0 <= search <= MAX_SEARCH:
        raise ValueError(f"search must be an integer in 0 .. {MAX_SEARCH}, not {search!r}")
    if min_echo is None:
        min_echo = int(block) * int(block) // 8
    if not _is_int(min_echo) or not 1 <= min_echo <= block * block:
        raise ValueError(f"min_echo must be an integer in 1 .. block * block = {block * block}, not {min_echo!r}")
    return int(block), int(stride), int(search), int(min_echo)


def _check_lattice(lattice) -> Lattice:
    try:
        oy, ox, sy, sx, ny, nx = lattice
        oy, ox, sy, sx = float(oy), float(ox), float(sy), float(sx)
    except (TypeError, ValueError):
        raise ValueError(f"lattice must be (origin_y, origin_x, step_y, step_x, ny, nx), got {lattice!r}") from None
    if not all(math.isfinite(v) for v in (oy, ox, sy, sx)) or sy <= 0.0 or sx <= 0.0:
        raise ValueError(f"lattice: origins must be finite and steps finite and positive, got {lattice!r}")
    if not (_is_int(ny) and _is_int(nx)) or ny < 1 or nx < 1:
        raise ValueError(f"lattice: ny and nx must be integers of at least 1, got {ny!r} and {nx!r}")
    return Lattice(oy, ox, sy, sx, int(ny), int(nx))


def _check_leads(leads) -> Tuple[float, ...]:
    try:
        leads = tuple(float(v) for v in (leads if hasattr(leads, "__iter__") else (leads,)))
    except (TypeError, ValueError):
        raise ValueError(f"leads must be numbers in units of the interval, got {leads!r}") from None
    if len(leads) > MAX_LEADS:
        raise ValueError(f"at most {MAX_LEADS} leads per call, got {len(leads)}")
    if not all(math.isfinite(v) for v in leads):
        raise ValueError(f"leads must be finite, got {leads!r}")
    return leads


def _check_sampling(method, substeps, fill_value, out, out_shape) -> float:
    """The advection's own arguments; returns the fill as a float."""
    if method not in ADVECT_METHODS:
        raise ValueError(f"method must be one of {sorted(ADVECT_METHODS)}, not {method!r}")
    if not _is_int(substeps) or not 1 <= substeps <= MAX_SUBSTEPS:
        raise ValueError(f"substeps must be an integer in 1 .. {MAX_SUBSTEPS}, not {substeps!r}")
    if out is not None and (not _is_tensor(out) or tuple(out.shape) != tuple(out_shape)):
        raise ValueError(f"out must be a tensor of shape {tuple(out_shape)}")
    return float(fill_value)


def _check_field(motion, lattice, plane_shape) -> Tuple[object, Lattice]:
    """The ``[ny, nx, 2]`` float32 field of ``motion`` (a :class:`MotionGrid` of one plane pair, a tensor or an ndarray) and
    its lattice."""
    if isinstance(motion, MotionGrid):
        if lattice is not None:
            raise ValueError("a MotionGrid carries its own lattice: pass lattice=None")
        if tuple(motion.shape) != tuple(plane_shape):
            raise ValueError(f"the MotionGrid was estimated on planes of {list(motion.shape)}, not {list(plane_shape)}")
        lattice, motion = motion.lattice, motion.motion
        if len(motion.shape) == 4:
            if int(motion.shape[0]) != 1:
                raise ValueError(f"advection takes the motion of ONE plane pair, not of {int(motion.shape[0])}: index the grid")
            motion = motion[0]
    if not hasattr(motion, "shape") or _dtype_name(motion) != "float32" or len(motion.shape) != 3 or int(motion.shape[2]) != 2:
        raise ValueError("motion must be a MotionGrid or float32 [ny, nx, 2] = (dy, dx)")
    ny, nx = int(motion.shape[0]), int(motion.shape[1])
    if lattice is None:
        if (ny, nx) != tuple(plane_shape):
            raise ValueError(f"motion of {[ny, nx]} nodes for planes of {list(plane_shape)} needs a lattice")
        lattice = Lattice(0.0, 0.0, 1.0, 1.0, ny, nx)
    lattice = _check_lattice(lattice)
    if (lattice.ny, lattice.nx) != (ny, nx):
        raise ValueError(f"lattice of {[lattice.ny, lattice.nx]} nodes for motion of {[ny, nx]}")
    if not _is_tensor(motion) and not np.isfinite(motion).all():
        raise ValueError("motion holds NaN or inf: fill it first (fill_motion_device)")
    return motion, lattice


# ---- device ------------------------------------------------------------------------------------------------------------------
def _to_device(a, dev, dtype=None):
    torch = _native.torch_mod()
    if not _is_tensor(a):
        a = np.ascontiguousarray(a)
        a = torch.from_numpy(a if a.flags.writeable else a.copy())          # torch takes no read-only array
    t = a
    if dtype is not None and t.dtype != dtype:
        t = (t != 0 if dtype == torch.uint8 else t).to(dtype)        # a mask of another type: non-zero excludes
    return t.to(dev).contiguous()


def _device_of(*arrays):
    for a in arrays:
        if a is not None and _is_tensor(a) and a.is_cuda:
            return a.device
    return _native.canonical_device(None)


def _quantize(lib, torch, src, mask_t, shape3, lo32, inv):
    out = torch.empty(shape3, dtype=torch.uint8, device=src.device)
    _native.check(lib.rg_motion_quantize_f32(_native.ptr(src), _native.ptr(mask_t), *shape3, lo32, inv, _native.ptr(out),
                                             _native.stream_ptr()), "rg_motion_quantize_f32")
    return out


def quantize_planes_device(planes, lo: float = 0.0, hi: float = 63.5, mask=None):
    """float32 planes ``[h, w]`` or ``[n, h, w]`` -> uint8 levels of the same shape (``rg_motion_quantize_f32``): 0 where
    ``mask`` is non-zero, the value is NaN or lies below ``lo``; otherwise ``1 + min(int((v - lo) * inv_step), 254)`` with
    ``inv_step = float32(254 / (hi - lo))`` -- 1 at ``lo``, 255 at ``hi`` and above.  The defaults span 0 .. 63.5 dBZ in
    quarter-dBZ levels."""
    shape3 = _check_planes(planes, "planes")
    lo32, inv = _check_levels(lo, hi)
    _check_mask(mask, planes, "mask")
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(planes, mask)
    src = _to_device(planes, dev)
    mask_t = None if mask is None else _to_device(mask, dev, torch.uint8)
    with torch.cuda.device(dev):
        out = _quantize(lib, torch, src, mask_t, shape3, lo32, inv)
    return out.reshape(tuple(planes.shape))


def estimate_motion_device(prev, next, *, block: int = 32, stride: int = 16, search: int = 16, lo: float = 0.0,
                           hi: float = 63.5, min_echo: Optional[int] = None, mask_prev=None, mask_next=None) -> MotionGrid:
    """One motion vector per block of ``prev``, searched within ``+-search`` pixels in ``next`` (``rg_block_match_u8``).

    ``prev`` / ``next``: planes of one shape, ``[h, w]`` or ``[n, h, w]`` (``n`` independent pairs; they may be ``q[:-1]`` and
    ``q[1:]`` of one stack), float32 -- quantised here with ``lo``, ``hi`` and the masks, see
    :func:`quantize_planes_device` -- or uint8 levels already quantised (masks are then a ``ValueError``).  A block of
    ``block`` x ``block`` pixels every ``stride`` pixels is valid with at least ``min_echo`` echo pixels (default
    ``block * block // 8``) and some contrast; its vector is the shift of the largest normalised cross-correlation (ties to the
    shortest shift), refined per axis by a parabola through the neighbouring scores.  Returns a :class:`MotionGrid`."""
    kinds = ("float32", "uint8")
    shape3 = _check_planes(prev, "prev", kinds)
    if _check_planes(next, "next", kinds) != shape3 or tuple(prev.shape) != tuple(next.shape):
        raise ValueError(f"prev of shape {list(prev.shape)} and next of shape {list(next.shape)} differ")
    if _dtype_name(prev) != _dtype_name(next):
        raise ValueError(f"prev is {_dtype_name(prev)} and next is {_dtype_name(next)}: quantise both or neither")
    block, stride, search, min_echo = _check_blocks(block, stride, search, min_echo)
    quantised = _dtype_name(prev) == "uint8"
    if quantised and (mask_prev is not None or mask_next is not None):
        raise ValueError("masks apply while float32 planes are quantised; these planes are uint8 levels already")
    lo32, inv = _check_levels(lo, hi)
    _check_mask(mask_prev, prev, "mask_prev")
    _check_mask(mask_next, next, "mask_next")
    n, h, w = shape3
    lat = block_lattice((h, w), block, stride)
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(prev, next)
    a, b = _to_device(prev, dev), _to_device(next, dev)
    with torch.cuda.device(dev):
        if not quantised:
            a = _quantize(lib, torch, a, None if mask_prev is None else _to_device(mask_prev, dev, torch.uint8), shape3, lo32, inv)
            b = _quantize(lib, torch, b, None if mask_next is None else _to_device(mask_next, dev, torch.uint8), shape3, lo32, inv)
        disp = torch.empty((n, lat.ny, lat.nx, 2), dtype=torch.int16, device=dev)
        motion = torch.empty((n, lat.ny, lat.nx, 2), dtype=torch.float32, device=dev)
        score = torch.empty((n, lat.ny, lat.nx), dtype=torch.float32, device=dev)
        _native.check(lib.rg_block_match_u8(_native.ptr(a), _native.ptr(b), n, h, w, block, stride, search, min_echo,
                                            _native.ptr(disp), _native.ptr(motion), _native.ptr(score), _native.stream_ptr()),
                      "rg_block_match_u8")
    if len(prev.shape) == 2:
        disp, motion, score = disp[0], motion[0], score[0]
    return MotionGrid(motion, score, disp, block, stride, search, (h, w), lat.origin_y, lat.step_y)


def fill_motion_device(grid: MotionGrid, min_score: float = 0.5) -> MotionGrid:
    """Replace the vectors of ``grid`` that are NaN, or whose score lies below ``min_score``, by the mean of the remaining
    vectors of the same plane pair (float64 sum, rounded once to float32); zero when none remains.  The result is finite
    everywhere, which :func:`advect_device` requires.

    Deliberately simple: a handful of torch elementwise operations and one reduction over a lattice of about 124 x 124 nodes
    -- no kernel of this package, no neighbourhood weighting, no smoothing.  No host synchronisation."""
    if not isinstance(grid, MotionGrid):
        raise ValueError(f"grid must be a MotionGrid, not {type(grid).__name__}")
    min_score = float(min_score)
    if math.isnan(min_score):
        raise ValueError("min_score must not be NaN")
    if not (_is_tensor(grid.motion) and _is_tensor(grid.score)) or len(grid.motion.shape) not in (3, 4):
        raise ValueError("grid.motion and grid.score must be the tensors estimate_motion_device returned")
    torch = _native.torch_mod()
    motion, score = grid.motion, grid.score
    good = (score >= min_score) & ~torch.isnan(motion).any(dim=-1)               # NaN scores compare false
    count = good.sum(dim=(-2, -1), keepdim=True).to(torch.float64)
    total = torch.where(good[..., None], motion.to(torch.float64), torch.zeros((), dtype=torch.float64, device=motion.device))
    total = total.sum(dim=(-3, -2), keepdim=True)
    mean = torch.where(count[..., None] > 0, total / count[..., None].clamp(min=1.0), torch.zeros_like(total)).to(torch.float32)
    return grid._replace(motion=torch.where(good[..., None], motion, mean.expand_as(motion)).contiguous())


def advect_device(planes, motion, leads, *, lattice=None, method: str = "nearest", substeps: int = 1,
                  fill_value: float = float("nan"), out=None):
    """Extrapolate ``planes`` along ``motion`` by each of ``leads`` intervals (``rg_advect_f32``).

    ``planes``: float32 ``[h, w]`` or ``[P, h, w]``; the result is ``[L, h, w]`` or ``[L, P, h, w]`` for ``L`` leads (at most
    16, in units of the interval between the two planes the motion was estimated from; a single number counts as one lead).
    ``motion``: a filled :class:`MotionGrid` of one plane pair, which carries its lattice, or float32 ``[ny, nx, 2]`` =
    ``(dy, dx)`` with ``lattice=(origin_y, origin_x, step_y, step_x, ny, nx)`` in pixels -- ``None`` means one vector per pixel.
    It must be finite everywhere (checked for an ndarray; for a tensor that is the caller's duty -- a NaN vector makes the
    pixels it reaches ``fill_value``).

    Backward semi-Lagrangian: for every output pixel ``p`` the displacement ``d`` is built in ``substeps`` (1 .. 16) steps,
    ``d += (lead / substeps) * V(p - d)`` with ``V`` the bilinear interpolant of the lattice (constant beyond its rim), and
    the pixel takes the plane's value at ``p - d``: ``method="nearest"`` copies the nearest pixel bit for bit,
    ``"bilinear"`` weights four, skips NaN and keeps the pixel while the present weights sum to at least 0.5 -- the warp's
    two rules.  Positions outside the plane give ``fill_value``.  One displacement serves all ``P`` planes.  ``out``: a
    contiguous float32 tensor of the result's shape on the device to write into (it must not overlap ``planes``)."""
    shape3 = _check_planes(planes, "planes")
    P, h, w = shape3
    field, lat = _check_field(motion, lattice, (h, w))
    leads = _check_leads(leads)
    out_shape = (len(leads), h, w) if len(planes.shape) == 2 else (len(leads), P, h, w)
    fill = _check_sampling(method, substeps, fill_value, out, out_shape)
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(planes, field)
    src = _to_device(planes, dev)
    field = _to_device(field, dev)
    if out is None:
        out = torch.empty(out_shape, dtype=torch.float32, device=dev)
    elif not (out.is_cuda and out.device == dev and out.dtype == torch.float32 and out.is_contiguous()):
        raise ValueError(f"out: expected a contiguous cuda float32 tensor on {dev}")
    if not leads:                                                            # an empty tensor has no address to pass
        return out
    c_leads = (_native.c_double * len(leads))(*leads)
    with torch.cuda.device(dev):
        _native.check(lib.rg_advect_f32(_native.ptr(src), P, h, w, _native.ptr(field), _native.MotionLattice(*lat), c_leads,
                                        len(leads), int(substeps), ADVECT_METHODS[method], fill, _native.ptr(out),
                                        _native.stream_ptr()), "rg_advect_f32")
    return out


def nowcast_device(prev, next, leads, *, min_score: float = 0.5, **kw):
    """``next`` extrapolated by ``leads`` intervals along the motion between ``prev`` and ``next`` (two float32 planes
    ``[h, w]``): :func:`estimate_motion_device` (which quantises), :func:`fill_motion_device` with ``min_score``, then
    :func:`advect_device` of ``next``.  Keywords go to the stage that names them (``block``, ``stride``, ``search``, ``lo``,
    ``hi``, ``min_echo``, ``mask_prev``, ``mask_next``; ``method``, ``substeps``, ``fill_value``, ``out``).  Returns
    ``(forecast [L, h, w], the filled MotionGrid)``, both on the device."""
    unknown = sorted(set(kw) - set(_ESTIMATE_KEYS) - set(_ADVECT_KEYS))
    if unknown:
        raise ValueError(f"unknown keyword(s) {unknown}: expected some of {list(_ESTIMATE_KEYS + _ADVECT_KEYS)}")
    for name, a in (("prev", prev), ("next", next)):
        if _check_planes(a, name)[0] != 1 or len(a.shape) != 2:
            raise ValueError(f"{name} must be one float32 [h, w] plane")
    leads = _check_leads(leads)
    if math.isnan(float(min_score)):
        raise ValueError("min_score must not be NaN")
    advect_kw = {k: v for k, v in kw.items() if k in _ADVECT_KEYS}
    _check_sampling(advect_kw.get("method", "nearest"), advect_kw.get("substeps", 1), advect_kw.get("fill_value", 0.0),
                    advect_kw.get("out"), (len(leads),) + tuple(int(v) for v in next.shape))
    grid = estimate_motion_device(prev, next, **{k: v for k, v in kw.items() if k in _ESTIMATE_KEYS})
    grid = fill_motion_device(grid, min_score)
    return advect_device(next, grid, leads, **advect_kw), grid


def nowcast(prev, next, leads, **kw):
    """:func:`nowcast_device` for NumPy arrays: ``(forecast float32 [L, h, w], MotionGrid of ndarrays)``."""
    forecast, grid = nowcast_device(prev, next, leads, **kw)
    return forecast.cpu().numpy(), grid._replace(motion=grid.motion.cpu().numpy(), score=grid.score.cpu().numpy(),
                                                 disp=grid.disp.cpu().numpy())


# ---- host --------------------------------------------------------------------------------------------------------------------
def motion_to_velocity(motion, geometry, interval_seconds: float):
    """Pixels per interval -> metres per second: ``(u_east, v_north)`` float64 arrays of ``motion``'s leading shape (host
    NumPy).  ``motion``: ``[.., 2]`` = ``(dy, dx)``, a :class:`MotionGrid`, tensor or ndarray; ``geometry`` names the grid the
    planes live on (``grid_shape`` and ``grid_limits``; the last two entries of each are read) -- a pixel is one grid step,
    ``(hi - lo) / (n - 1)`` metres, row index growing northwards; ``interval_seconds`` is the time between the two planes."""
    interval = float(interval_seconds)
    if not (math.isfinite(interval) and interval > 0.0):
        raise ValueError(f"interval_seconds must be finite and positive, not {interval_seconds!r}")
    try:
        ny, nx = (int(v) for v in tuple(geometry.grid_shape)[-2:])
        (y_lo, y_hi), (x_lo, x_hi) = ((float(a), float(b)) for a, b in tuple(geometry.grid_limits)[-2:])
    except (AttributeError, TypeError, ValueError):
        raise ValueError("geometry must carry grid_shape and grid_limits") from None
    if ny < 2 or nx < 2 or not all(math.isfinite(v) for v in (y_lo, y_hi, x_lo, x_hi)) or y_hi <= y_lo or x_hi <= x_lo:
        raise ValueError(f"geometry: at least 2 x 2 nodes between finite, increasing limits; got {[ny, nx]}")
    if isinstance(motion, MotionGrid):
        if tuple(motion.shape) != (ny, nx):
            raise ValueError(f"the MotionGrid was estimated on planes of {list(motion.shape)}, the geometry has {[ny, nx]}")
        motion = motion.motion
    m = (motion.detach().cpu().numpy() if _is_tensor(motion) else np.asarray(motion)).astype(np.float64)
    if m.ndim < 1 or m.shape[-1] != 2:
        raise ValueError(f"motion must be [.., 2] = (dy, dx), got {list(m.shape)}")
    step_y, step_x = (y_hi - y_lo) / (ny - 1), (x_hi - x_lo) / (nx - 1)
    return m[..., 1] * step_x / interval, m[..., 0] * step_y / interval
