"""Rain rate and advection-corrected rainfall accumulation on the device (include/radargrid_hip.h, "Rain rate and
accumulation"; kernels in csrc/rg_accumulate.hip): how hard it rains now, and how much fell over the last interval or hour.

* :func:`rain_rate_device` turns dBZ planes into mm/h under ``Z = a R^b`` (``rg_rain_rate_f32``);
* :func:`accumulate_device` sums the interval between two rate planes ALONG the echo's motion
  (``rg_accumulate_advected_f32``), so that a cell moving several pixels per scan leaves a swath instead of one blob per scan;
  :func:`accumulate` is its NumPy-in, NumPy-out wrapper;
* :class:`RainAccumulator` chains the two with the motion estimate of :mod:`.motion` over a sequence of scans and keeps the
  running total of a time window -- what :class:`~radar_processor_amd.tracking.CellTracker` is for cells.

A rate plane has three kinds of pixel: NaN = no coverage, 0 = covered and dry, > 0 = rain.  Motion, its sign and its units are
those of :mod:`.motion`: ``(dy, dx)`` in pixels per interval, from the earlier plane to the later one.

The device functions take tensors or ndarrays, enqueue on torch's current stream, validate every argument before the device
is touched and never synchronise with the host.  The accumulation kernel is pinned bit for bit to the NumPy restatement of
the header's formulas (``tests/accumulation_oracle.py``), the rate kernel to one float32 step of it.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np

from . import _native
from .motion import (_ESTIMATE_KEYS, ADVECT_METHODS, MAX_SUBSTEPS, Lattice, MotionGrid, _check_blocks, _check_field, _check_levels,
                     _check_mask, _check_planes, _device_of, _is_int, _is_tensor, _to_device, estimate_motion_device,
                     fill_motion_device)

MAX_STEPS = _native.RG_MAX_ACC_STEPS
_TRACKER_ESTIMATE_KEYS = tuple(k for k in _ESTIMATE_KEYS if not k.startswith("mask_"))      # the masks come with the frames


class AccumulationFrame(NamedTuple):
    """What :meth:`RainAccumulator.update` returns, everything on the device.  ``rate`` float32 ``[h, w]`` mm/h of this scan;
    ``interval_mm`` the depth since the previous scan, ``None`` for the first scan and after a gap; ``total_mm`` the depth over
    the accumulator's window, ``None`` while it holds no interval; ``motion`` the filled :class:`MotionGrid` (or the given
    field, or ``None``) the interval was summed along; ``seconds`` the length of the interval (``None`` without one)."""
    rate: object
    interval_mm: object
    total_mm: object
    motion: object
    seconds: Optional[float]


# ---- validation (host only) --------------------------------------------------------------------------------------------------
def _check_zr(a, b, min_dbz, max_dbz):
    """``(p, q, min_dbz, max_dbz)`` as the doubles the kernel takes: ``R = exp(dBZ * p - q)``."""
    try:
        a, b, min_dbz, max_dbz = float(a), float(b), float(min_dbz), float(max_dbz)
    except (TypeError, ValueError):
        raise ValueError(f"a, b, min_dbz and max_dbz must be numbers, got {(a, b, min_dbz, max_dbz)!r}") from None
    if not (math.isfinite(a) and math.isfinite(b)) or a <= 0.0 or b <= 0.0:
        raise ValueError(f"Z = a R^b needs finite a > 0 and b > 0, got a={a!r} and b={b!r}")
    if not (math.isfinite(min_dbz) and math.isfinite(max_dbz)) or max_dbz < min_dbz:
        raise ValueError(f"min_dbz and max_dbz must be finite with max_dbz >= min_dbz, got {min_dbz!r} and {max_dbz!r}")
    p, q = math.log(10.0) / (10.0 * b), math.log(a) / b
    if not (math.isfinite(p) and p > 0.0 and math.isfinite(q)):
        raise ValueError(f"a={a!r} and b={b!r} leave no finite rate")
    return p, q, min_dbz, max_dbz


def _check_hours(hours) -> float:
    try:
        hours = float(hours)
    except (TypeError, ValueError):
        raise ValueError(f"hours must be a number, not {hours!r}") from None
    if not (math.isfinite(hours) and hours > 0.0):
        raise ValueError(f"hours must be finite and positive, not {hours!r}")
    return hours


def _check_steps(steps, substeps, min_steps, method):
    if not _is_int(steps) or not 1 <= steps <= MAX_STEPS:
        raise ValueError(f"steps must be an integer in 1 .. {MAX_STEPS}, not {steps!r}")
    if not _is_int(substeps) or not 1 <= substeps <= MAX_SUBSTEPS:
        raise ValueError(f"substeps must be an integer in 1 .. {MAX_SUBSTEPS}, not {substeps!r}")
    if min_steps is None:
        min_steps = steps
    if not _is_int(min_steps) or not 1 <= min_steps <= steps:
        raise ValueError(f"min_steps must be an integer in 1 .. steps = {steps}, not {min_steps!r}")
    if method not in ADVECT_METHODS:
        raise ValueError(f"method must be one of {sorted(ADVECT_METHODS)}, not {method!r}")
    return int(steps), int(substeps), int(min_steps)


# ---- device ------------------------------------------------------------------------------------------------------------------
def rain_rate_device(planes, *, a: float = 200.0, b: float = 1.6, min_dbz: float = 5.0, max_dbz: float = 55.0, mask=None):
    """dBZ planes ``[h, w]`` or ``[n, h, w]`` (float32) -> mm/h of the same shape under ``Z = a R^b`` (``rg_rain_rate_f32``);
    the defaults are Marshall-Palmer.  NaN where ``mask`` is non-zero or the value is NaN (no coverage); 0 below ``min_dbz``
    (covered, dry; -inf included); otherwise ``exp(min(dBZ, max_dbz) * p - q)`` in float64 with ``p = ln(10) / (10 b)`` and
    ``q = ln(a) / b``, rounded once to float32 -- ``max_dbz`` caps hail."""
    shape3 = _check_planes(planes, "planes")
    p, q, min_dbz, max_dbz = _check_zr(a, b, min_dbz, max_dbz)
    _check_mask(mask, planes, "mask")
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(planes, mask)
    src = _to_device(planes, dev)
    mask_t = None if mask is None else _to_device(mask, dev, torch.uint8)
    out = torch.empty(shape3, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _native.check(lib.rg_rain_rate_f32(_native.ptr(src), _native.ptr(mask_t), *shape3, p, q, min_dbz, max_dbz, _native.ptr(out),
                                           _native.stream_ptr()), "rg_rain_rate_f32")
    return out.reshape(tuple(planes.shape))


def accumulate_device(rate_prev, rate_next, motion, hours: float, *, steps: int, lattice=None, method: str = "bilinear",
                      substeps: int = 1, min_steps: Optional[int] = None, fill_value: float = float("nan"),
                      return_steps: bool = False, out=None):
    """The depth that fell between two rate planes ``hours`` apart, summed along ``motion``
    (``rg_accumulate_advected_f32``).

    ``rate_prev`` / ``rate_next``: float32 ``[h, w]`` or ``[P, h, w]`` of one shape, the rates at the two ends of the
    interval; the result has that shape, in rate unit times hours (mm for mm/h).  ``motion``: the motion from prev to next --
    a filled :class:`MotionGrid` of one plane pair, or float32 ``[ny, nx, 2]`` = ``(dy, dx)`` with ``lattice``, exactly as
    for :func:`~radar_processor_amd.motion.advect_device`; ``None`` is zero motion, the plain blend in time.

    The interval is cut into ``steps`` (1 .. 64) sub-instants ``s = (k + 0.5) / steps``.  At each one the pixel takes
    ``rate_prev`` moved forward by ``s`` intervals and ``rate_next`` moved backward by ``1 - s`` -- the two samples
    :func:`advect_device` would give for the leads ``s`` and ``s - 1`` with ``method`` and ``substeps`` -- and blends them
    ``(1 - s) * a + s * b``.  A sample that is NaN (outside the plane, no coverage) is missing: the other one stands alone;
    with both missing the step is missing.  The pixel is ``hours`` times the mean of its present steps when there are at
    least ``min_steps`` of them (default: all ``steps``), else ``fill_value``.  Choose ``steps`` so that a step moves the echo
    by about a pixel: fewer leave gaps between the deposits of a fast cell.

    ``return_steps=True`` also returns the uint8 count of present steps per pixel.  ``out``: a contiguous float32 tensor of the
    result's shape on the device to write into (it must not overlap an input)."""
    shape3 = _check_planes(rate_prev, "rate_prev")
    if _check_planes(rate_next, "rate_next") != shape3 or tuple(rate_prev.shape) != tuple(rate_next.shape):
        raise ValueError(f"rate_prev of shape {list(rate_prev.shape)} and rate_next of shape {list(rate_next.shape)} differ")
    P, h, w = shape3
    if motion is None:
        if lattice is not None:
            raise ValueError("motion=None is zero motion: pass lattice=None")
        field, lat = None, Lattice(0.0, 0.0, 1.0, 1.0, 1, 1)
    else:
        field, lat = _check_field(motion, lattice, (h, w))
    hours = _check_hours(hours)
    steps, substeps, min_steps = _check_steps(steps, substeps, min_steps, method)
    out_shape = tuple(int(v) for v in rate_prev.shape)
    if out is not None and (not _is_tensor(out) or tuple(out.shape) != out_shape):
        raise ValueError(f"out must be a tensor of shape {out_shape}")
    fill = float(fill_value)
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(rate_prev, rate_next, field)
    a, b = _to_device(rate_prev, dev), _to_device(rate_next, dev)
    field = torch.zeros((1, 1, 2), dtype=torch.float32, device=dev) if field is None else _to_device(field, dev)
    if out is None:
        out = torch.empty(out_shape, dtype=torch.float32, device=dev)
    elif not (out.is_cuda and out.device == dev and out.dtype == torch.float32 and out.is_contiguous()):
        raise ValueError(f"out: expected a contiguous cuda float32 tensor on {dev}")
    count = torch.empty(out_shape, dtype=torch.uint8, device=dev) if return_steps else None
    with torch.cuda.device(dev):
        _native.check(lib.rg_accumulate_advected_f32(_native.ptr(a), _native.ptr(b), P, h, w, _native.ptr(field),
                                                     _native.MotionLattice(*lat), hours, steps, substeps, ADVECT_METHODS[method],
                                                     min_steps, fill, _native.ptr(out), _native.ptr(count), _native.stream_ptr()),
                      "rg_accumulate_advected_f32")
    return (out, count) if return_steps else out


def accumulate(rate_prev, rate_next, motion, hours, **kw):
    """:func:`accumulate_device` for NumPy arrays: the float32 depth, or ``(depth, uint8 steps)`` with ``return_steps=True``."""
    result = accumulate_device(rate_prev, rate_next, motion, hours, **kw)
    if isinstance(result, tuple):
        return tuple(r.cpu().numpy() for r in result)
    return result.cpu().numpy()


class RainAccumulator:
    """Rainfall over a sequence of scans: feed it one dBZ plane per scan, read the rate, the depth of the last interval and
    the depth over a time window.

    ``a``, ``b``, ``min_dbz``, ``max_dbz``: the Z-R conversion of :func:`rain_rate_device`.  ``motion``: ``"auto"`` estimates
    the motion between the previous and the current dBZ plane (:func:`estimate_motion_device`, then
    :func:`fill_motion_device` with ``min_score``; further keywords -- ``block``, ``stride``, ``search``, ``lo``, ``hi``,
    ``min_echo`` -- go to the estimate); ``None`` is zero motion; a filled :class:`MotionGrid` or a ``(field, lattice)`` pair is
    used as it is for every interval.  ``steps``: sub-instants per interval, see :func:`accumulate_device`; ``None`` means the
    estimate's ``search`` under ``"auto"`` -- no vector is longer, so a step moves the echo by at most about a pixel and
    nothing has to be read back -- and 1 without motion.  ``window_seconds``: how far back :meth:`total` reaches, and how long
    an interval is kept.  ``max_gap_seconds``: two scans further apart are not joined.  ``convective_zr``: an ``(a, b)`` pair
    for the convective pixels -- every scan is then classified (:func:`~radar_processor_amd.convection.convective_stratiform_device`
    with the keywords of ``classify``, which must hold the spacing: ``dx`` / ``dy`` or ``geometry``) and ``a``, ``b`` stay the
    stratiform relation (:func:`~radar_processor_amd.convection.rain_rate_by_class_device`); ``None`` (the default) classifies
    nothing and applies ``a``, ``b`` everywhere.

    Nothing here synchronises with the host."""

    def __init__(self, *, a: float = 200.0, b: float = 1.6, min_dbz: float = 5.0, max_dbz: float = 55.0, motion="auto",
                 steps: Optional[int] = None, method: str = "bilinear", window_seconds: float = 3600.0,
                 max_gap_seconds: float = 900.0, min_score: float = 0.5, convective_zr=None, classify: Optional[dict] = None,
                 **estimate):
        _check_zr(a, b, min_dbz, max_dbz)
        self._zr = dict(a=float(a), b=float(b), min_dbz=float(min_dbz), max_dbz=float(max_dbz))
        self._convective_zr, self._classify = None, None
        if convective_zr is not None:
            from .convection import _check_classify                  # convection imports this module
            try:
                conv_a, conv_b = convective_zr
            except (TypeError, ValueError):
                raise ValueError(f"convective_zr must be an (a, b) pair, not {convective_zr!r}") from None
            _check_zr(conv_a, conv_b, min_dbz, max_dbz)
            self._convective_zr, self._classify = (float(conv_a), float(conv_b)), _check_classify(classify)
        elif classify is not None:
            raise ValueError("classify holds the keywords of the classification, which runs only with convective_zr")
        unknown = sorted(set(estimate) - set(_TRACKER_ESTIMATE_KEYS))
        if unknown:
            raise ValueError(f"unknown keyword(s) {unknown}: expected some of {list(_TRACKER_ESTIMATE_KEYS)}")
        self._lattice = None
        if isinstance(motion, str):
            if motion != "auto":
                raise ValueError(f"motion must be 'auto', None, a MotionGrid or (field, lattice), not {motion!r}")
            _, _, search, _ = _check_blocks(estimate.get("block", 32), estimate.get("stride", 16), estimate.get("search", 16),
                                            estimate.get("min_echo"))
            _check_levels(estimate.get("lo", 0.0), estimate.get("hi", 63.5))
            default_steps = max(search, 1)
        else:
            if estimate:
                raise ValueError(f"{sorted(estimate)} belong to the motion estimate, which motion={type(motion).__name__} does not run")
            if isinstance(motion, tuple) and not isinstance(motion, MotionGrid):
                if len(motion) != 2:
                    raise ValueError("a given motion is a MotionGrid or the pair (field, lattice)")
                motion, self._lattice = motion
            if motion is not None and not isinstance(motion, MotionGrid) and not hasattr(motion, "shape"):
                raise ValueError(f"motion must be 'auto', None, a MotionGrid or (field, lattice), not {type(motion).__name__}")
            default_steps = 1 if motion is None else None
        if steps is None:
            if default_steps is None:
                raise ValueError("steps is required with a given motion field: about its longest vector in pixels")
            steps = default_steps
        self.steps, _, _ = _check_steps(steps, 1, None, method)
        self.method = method
        self.motion = motion
        self._estimate = dict(estimate)
        self.min_score = float(min_score)
        if math.isnan(self.min_score):
            raise ValueError("min_score must not be NaN")
        self.window_seconds, self.max_gap_seconds = float(window_seconds), float(max_gap_seconds)
        if not (math.isfinite(self.window_seconds) and self.window_seconds > 0.0):
            raise ValueError(f"window_seconds must be finite and positive, not {window_seconds!r}")
        if not self.max_gap_seconds > 0.0:
            raise ValueError(f"max_gap_seconds must be positive, not {max_gap_seconds!r}")
        self.reset()

    def reset(self) -> None:
        """Forget every scan and interval."""
        self._last = None                    # (seconds, dBZ tensor, mask tensor or None, rate tensor)
        self._intervals = []                 # [(end seconds, depth tensor)], in time order

    @property
    def intervals(self):
        """``[(end time in seconds, float32 depth [h, w])]`` of the kept intervals, oldest first."""
        return list(self._intervals)

    def update(self, plane_dbz, time_seconds: float, mask=None) -> AccumulationFrame:
        """Take the scan of ``time_seconds``: ``plane_dbz`` float32 ``[h, w]``, ``mask`` (optional) non-zero where the radar
        does not see.  Converts it to a rate, finds the motion since the previous scan, accumulates the interval between the
        two and returns an :class:`AccumulationFrame`.  ``ValueError`` for a time that does not increase.  A scan more than
        ``max_gap_seconds`` after the previous one accumulates nothing and empties the window."""
        if _check_planes(plane_dbz, "plane_dbz")[0] != 1 or len(plane_dbz.shape) != 2:
            raise ValueError("plane_dbz must be one float32 [h, w] plane")
        _check_mask(mask, plane_dbz, "mask")
        try:
            now = float(time_seconds)
        except (TypeError, ValueError):
            raise ValueError(f"time_seconds must be a number, not {time_seconds!r}") from None
        if not math.isfinite(now):
            raise ValueError(f"time_seconds must be finite, not {time_seconds!r}")
        if self._last is not None:
            if not now > self._last[0]:
                raise ValueError(f"time_seconds must increase: {now!r} after {self._last[0]!r}")
            if tuple(self._last[1].shape) != tuple(int(v) for v in plane_dbz.shape):
                raise ValueError(f"plane_dbz of shape {list(plane_dbz.shape)} after planes of {list(self._last[1].shape)}")
        torch = _native.torch_mod()
        dev = _device_of(plane_dbz, mask) if self._last is None else self._last[1].device
        dbz = _to_device(plane_dbz, dev)
        mask_t = None if mask is None else _to_device(mask, dev, torch.uint8)
        if self._convective_zr is None:
            rate = rain_rate_device(dbz, mask=mask_t, **self._zr)
        else:
            from .convection import convective_stratiform_device, rain_rate_by_class_device
            classes = convective_stratiform_device(dbz, mask=mask_t, **self._classify)
            rate = rain_rate_by_class_device(dbz, classes, stratiform=(self._zr["a"], self._zr["b"]), convective=self._convective_zr,
                                             min_dbz=self._zr["min_dbz"], max_dbz=self._zr["max_dbz"], mask=mask_t)
        last, self._last = self._last, (now, dbz, mask_t, rate)
        if last is None or now - last[0] > self.max_gap_seconds:
            self._intervals = []
            return AccumulationFrame(rate, None, None, None, None)
        seconds = now - last[0]
        if isinstance(self.motion, str):
            grid = estimate_motion_device(last[1], dbz, mask_prev=last[2], mask_next=mask_t, **self._estimate)
            motion, lattice = fill_motion_device(grid, self.min_score), None
        else:
            motion, lattice = self.motion, self._lattice
        depth = accumulate_device(last[3], rate, motion, seconds / 3600.0, steps=self.steps, lattice=lattice, method=self.method)
        self._intervals = [(end, d) for end, d in self._intervals if end > now - self.window_seconds] + [(now, depth)]
        return AccumulationFrame(rate, depth, self.total(), motion, seconds)

    def total(self, window_seconds: Optional[float] = None, skip_missing: bool = False):
        """The depth over the last ``window_seconds`` (default: the accumulator's window) before the latest scan: the kept
        intervals whose END lies less than that before it, summed in float64 in time order and cast once to float32.  A pixel
        that is NaN in one of them is NaN in the sum, unless ``skip_missing`` -- then a NaN adds nothing (the sum of the
        intervals that do cover the pixel; 0 where none does).  ``None`` while no interval is kept."""
        window = self.window_seconds if window_seconds is None else float(window_seconds)
        if not window > 0.0:
            raise ValueError(f"window_seconds must be positive, not {window_seconds!r}")
        if self._last is None or not self._intervals:
            return None
        torch = _native.torch_mod()
        total = None
        for end, depth in self._intervals:
            if not end > self._last[0] - window:
                continue
            v = depth.to(torch.float64)
            if skip_missing:
                v = torch.where(torch.isnan(v), torch.zeros((), dtype=torch.float64, device=v.device), v)
            total = v if total is None else total + v
        return None if total is None else total.to(torch.float32)
