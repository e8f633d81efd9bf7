"""Azimuthal shear and radial divergence of the Doppler velocity by local linear least squares (LLSD), on the device
(include/radargrid_shear.h; kernels in csrc/rg_shear.hip): what a dealiased velocity is for.  Azimuthal shear is the quantity
rotation tracks and mesocyclone detection are built on; radial divergence shows downbursts and convergence lines.

* :func:`llsd_window` turns the geometry of a sweep into the window tables of the fit (host, float64, no device);
* :func:`median_filter_device` is the small median filter that precedes the LLSD (``rg_polar_median_f32``);
* :func:`velocity_shear_device` fits a plane to the velocities of a (ray, gate) window whose azimuthal extent changes with
  range and returns its two slopes as shear and divergence, the fitted velocity and the count (``rg_velocity_llsd_f32``);
* :func:`azimuthal_shear_device` chains the two; :func:`velocity_shear` is the NumPy-in, NumPy-out form.

A volume is float32 ``[n_sweeps, n_rays, n_gates]`` (tensor or ndarray); a 2-D input is one sweep.  It takes
``DealiasedVelocity.velocity`` as it comes, and ``azimuthal_shear.reshape(-1)`` is what ``fields`` of the gridders take.

The method is that of Smith & Elmore (2004) and Mahalik et al. (2019), restated so that every sum is an integer in 2^-16 m/s
fixed point.  The fit is in index coordinates: all gates of a window share the centre gate's arc length per ray, and the rays
of a sweep are taken as equally spaced.  The contract is this build's own (the header states it; ``tests/shear_oracle.py``
restates it in NumPy and the tests hold the kernels EQUAL to that, bit for bit).  Parity with WDSS-II / LROSE / PyART is
unpinned.  The device functions enqueue on torch's current stream, never synchronise with the host and validate every argument
before the device is touched.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _native
from .motion import _device_of, _dtype_name, _is_int, _to_device
from .velocity import _check_like, _check_volume

MEDIAN_MAX_HALF = _native.RG_SHEAR_MEDIAN_MAX_HALF
MAX_HALF_RAYS = _native.RG_SHEAR_MAX_HALF_RAYS
MAX_HALF_GATES = _native.RG_SHEAR_MAX_HALF_GATES
MAX_WINDOW = _native.RG_SHEAR_MAX_WINDOW
PRODUCTS = ("azimuthal_shear", "radial_divergence", "velocity", "count")


class ShearWindow(NamedTuple):
    """The window of the LLSD: ``half_rays`` int32 ``[n_gates]`` (rays on either side of the centre, per gate index),
    ``az_scale`` float64 ``[n_gates]`` (``1 / (65536 r dtheta)``: fixed point per ray step -> 1/s), ``max_half_rays`` (the clamp
    of ``half_rays``, and what the circle of rays has to hold under ``wrap_rays``), ``half_gates`` and ``range_scale``
    (``1 / (65536 dr)``).  Any tables are accepted by the device call: :func:`llsd_window` is one way to make them."""
    half_rays: object
    az_scale: object
    max_half_rays: int
    half_gates: int
    range_scale: float


class VelocityShear(NamedTuple):
    """What :func:`velocity_shear_device` returns, each of the input's shape or ``None`` when not asked for: ``azimuthal_shear``
    and ``radial_divergence`` float32 in 1/s, ``velocity`` float32 (the fitted plane at the centre gate, m/s), all NaN where the
    fit is not defined, and ``count`` uint16 (valid gates of the window, written everywhere; torch reduces few things over
    uint16: ``count.to(torch.int32)`` first)."""
    azimuthal_shear: object
    radial_divergence: object
    velocity: object
    count: object


# ---- host --------------------------------------------------------------------------------------------------------------------
def llsd_window(ranges_m, ray_spacing_deg: float, gate_spacing_m: float, *, azimuthal_width_m: float = 2500.0,
                range_width_m: float = 750.0, min_half_rays: int = 1, max_half_rays: int = MAX_HALF_RAYS) -> ShearWindow:
    """The window tables for gates at ``ranges_m`` (metres, one per gate index) of rays ``ray_spacing_deg`` apart and gates
    ``gate_spacing_m`` apart, so that a window is about ``azimuthal_width_m`` across the beam and ``range_width_m`` along it:

    * ``half_rays[g] = clip(floor(azimuthal_width_m / (2 r dtheta) + 0.5), min_half_rays, max_half_rays)``;
    * ``half_gates = clip(floor(range_width_m / (2 dr) + 0.5), 1, 16)``;
    * ``az_scale[g] = 1 / (65536 r dtheta)`` and ``range_scale = 1 / (65536 dr)``, ``dtheta`` in radians;
    * a gate with ``r <= 0`` gets ``half_rays = 0`` and ``az_scale = 0``: its fit is never defined.

    Host code in float64; needs no device."""
    r = np.asarray(ranges_m, dtype=np.float64)
    if r.ndim != 1 or not np.isfinite(r).all():
        raise ValueError(f"ranges_m must be a 1-D array of finite ranges, got shape {list(r.shape)}")
    for name, value in (("ray_spacing_deg", ray_spacing_deg), ("gate_spacing_m", gate_spacing_m),
                        ("azimuthal_width_m", azimuthal_width_m), ("range_width_m", range_width_m)):
        if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or not (
                math.isfinite(value) and value > 0.0):
            raise ValueError(f"{name} must be a finite number above 0, not {value!r}")
    if not _is_int(max_half_rays) or not 1 <= max_half_rays <= MAX_HALF_RAYS:
        raise ValueError(f"max_half_rays must be an integer in 1 .. {MAX_HALF_RAYS}, not {max_half_rays!r}")
    if not _is_int(min_half_rays) or not 0 <= min_half_rays <= max_half_rays:
        raise ValueError(f"min_half_rays must be an integer in 0 .. max_half_rays, not {min_half_rays!r}")
    dtheta = float(ray_spacing_deg) * (math.pi / 180.0)
    arc = r * dtheta                                                    # metres per ray step
    ok = r > 0.0
    safe = np.where(ok, arc, 1.0)
    half = np.clip(np.floor(float(azimuthal_width_m) / (2.0 * safe) + 0.5), int(min_half_rays), int(max_half_rays))
    half_rays = np.where(ok, half, 0.0).astype(np.int32)
    az_scale = np.where(ok, 1.0 / (65536.0 * safe), 0.0)
    half_gates = int(min(max(math.floor(float(range_width_m) / (2.0 * float(gate_spacing_m)) + 0.5), 1), MAX_HALF_GATES))
    return ShearWindow(half_rays, az_scale, int(max_half_rays), half_gates, 1.0 / (65536.0 * float(gate_spacing_m)))


# ---- validation (host only) --------------------------------------------------------------------------------------------------
def _check_size(vel, shape3) -> None:
    if shape3[0] * shape3[1] * shape3[2] >= 2 ** 31:
        raise ValueError(f"vel: {list(vel.shape)} holds 2^31 gates or more: split the volume by sweeps")


def _check_flag_int(value, lo: int, hi: int, what: str) -> int:
    if not _is_int(value) or not lo <= value <= hi:
        raise ValueError(f"{what} must be an integer in {lo} .. {hi}, not {value!r}")
    return int(value)


def _check_median(shape3, half_rays, half_gates, wrap_rays, min_valid) -> Tuple[int, int, int]:
    half_rays = _check_flag_int(half_rays, 0, MEDIAN_MAX_HALF, "half_rays")
    half_gates = _check_flag_int(half_gates, 0, MEDIAN_MAX_HALF, "half_gates")
    if half_rays == 0 and half_gates == 0:
        raise ValueError("half_rays and half_gates are both 0: the median of one gate is the gate")
    if wrap_rays and 2 * half_rays + 1 > shape3[1]:
        raise ValueError(f"a median window of {2 * half_rays + 1} rays does not fit a circle of {shape3[1]} rays (wrap_rays)")
    return half_rays, half_gates, _check_flag_int(min_valid, 1, 25, "min_valid")


def _check_window(window, shape3, wrap_rays) -> ShearWindow:
    if not isinstance(window, tuple) or len(window) != 5:
        raise ValueError("window must be a ShearWindow (half_rays, az_scale, max_half_rays, half_gates, range_scale)")
    window = ShearWindow(*window)
    G = shape3[2]
    for table, dtype, name in ((window.half_rays, "int32", "half_rays"), (window.az_scale, "float64", "az_scale")):
        if not hasattr(table, "shape") or _dtype_name(table) != dtype or tuple(int(n) for n in table.shape) != (G,):
            raise ValueError(f"window.{name} must be {dtype} [{G}] (one entry per gate index), got "
                             f"{_dtype_name(table) if hasattr(table, 'dtype') else type(table).__name__} "
                             f"{list(getattr(table, 'shape', []))}")
    max_half_rays = _check_flag_int(window.max_half_rays, 1, MAX_HALF_RAYS, "window.max_half_rays")
    half_gates = _check_flag_int(window.half_gates, 1, MAX_HALF_GATES, "window.half_gates")
    scale = window.range_scale
    if isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)) or not math.isfinite(scale):
        raise ValueError(f"window.range_scale must be a finite number, not {scale!r}")
    if wrap_rays and 2 * max_half_rays + 1 > shape3[1]:
        raise ValueError(f"a window of {2 * max_half_rays + 1} rays (max_half_rays = {max_half_rays}) does not fit a circle of "
                         f"{shape3[1]} rays (wrap_rays): lower max_half_rays or pass wrap_rays=False")
    return ShearWindow(window.half_rays, window.az_scale, max_half_rays, half_gates, float(scale))


def _check_fit(min_valid, min_fraction, want) -> Tuple[int, int, Tuple[str, ...]]:
    min_valid = _check_flag_int(min_valid, 3, MAX_WINDOW, "min_valid")
    if isinstance(min_fraction, bool) or not isinstance(min_fraction, (int, float, np.integer, np.floating)) or not (
            0.0 <= min_fraction <= 1.0):
        raise ValueError(f"min_fraction must be a number in 0 .. 1, not {min_fraction!r}")
    if isinstance(want, str) or not isinstance(want, Sequence) or any(w not in PRODUCTS for w in want):
        raise ValueError(f"want must be a sequence of names out of {PRODUCTS}, not {want!r}")
    if not any(w in PRODUCTS[:3] for w in want):
        raise ValueError(f"want must name at least one of {PRODUCTS[:3]}, not {want!r}")
    return min_valid, int(math.floor(float(min_fraction) * 65536.0 + 0.5)), tuple(want)


# ---- device ------------------------------------------------------------------------------------------------------------------
def _median(lib, torch, src, m, shape3, half_rays, half_gates, wrap_rays, min_valid, centre_only):
    S, R, G = shape3
    out = torch.empty(shape3, dtype=torch.float32, device=src.device)
    if G:                        # rays without gates: the empty output is the result (and an empty tensor has no address)
        _native.check(lib.rg_polar_median_f32(_native.ptr(src), _native.ptr(m), S, R, G, half_rays, half_gates, 1 if wrap_rays else 0,
                                              min_valid, 1 if centre_only else 0, _native.ptr(out), _native.stream_ptr()),
                      "rg_polar_median_f32")
    return out


def _llsd(lib, torch, src, m, shape3, window: ShearWindow, tables, wrap_rays, min_valid, min_fraction_q16, centre_only, want):
    S, R, G = shape3
    dev = src.device
    outs = [torch.empty(shape3, dtype=torch.float32, device=dev) if name in want else None for name in PRODUCTS[:3]]
    count = torch.empty(shape3, dtype=torch.uint16, device=dev) if "count" in want else None
    if G:
        _native.check(lib.rg_velocity_llsd_f32(_native.ptr(src), _native.ptr(m), S, R, G, _native.ptr(tables[0]), _native.ptr(tables[1]),
                                               window.max_half_rays, window.half_gates, window.range_scale, 1 if wrap_rays else 0,
                                               min_valid, min_fraction_q16, 1 if centre_only else 0, _native.ptr(outs[0]),
                                               _native.ptr(outs[1]), _native.ptr(outs[2]), _native.ptr(count), _native.stream_ptr()),
                      "rg_velocity_llsd_f32")
    return outs + [count]


def _stage(vel, mask, extra=()):
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(vel, mask, *extra)
    src = _to_device(vel, dev)
    m = None if mask is None else _to_device(mask, dev, torch.uint8)
    return torch, lib, dev, src, m


def median_filter_device(vel, *, half_rays: int = 1, half_gates: int = 1, mask=None, wrap_rays: bool = True, min_valid: int = 1,
                         centre_only: bool = True):
    """The lower median of the valid gates in a window of ``(2 half_rays + 1) x (2 half_gates + 1)`` gates (each half-width 0,
    1 or 2, not both 0) around every gate: float32 of the volume's shape on the device.  A selection, never an average: an output
    is one of the inputs, bit for bit.  NaN where the window holds fewer than ``min_valid`` valid gates, and, with
    ``centre_only``, where the centre gate itself is not valid (the filter then removes outliers but fills no holes).  With
    ``wrap_rays`` every sweep is a full circle.  No host synchronisation."""
    shape3 = _check_volume(vel, "vel")
    _check_size(vel, shape3)
    half_rays, half_gates, min_valid = _check_median(shape3, half_rays, half_gates, wrap_rays, min_valid)
    _check_like(mask, vel, "mask", None)
    torch, lib, dev, src, m = _stage(vel, mask)
    with torch.cuda.device(dev):
        out = _median(lib, torch, src, m, shape3, half_rays, half_gates, wrap_rays, min_valid, centre_only)
    return out.reshape(tuple(vel.shape))


def velocity_shear_device(vel, window, *, mask=None, wrap_rays: bool = True, min_valid: int = 6, min_fraction: float = 0.5,
                          centre_only: bool = False, want=("azimuthal_shear", "radial_divergence")) -> VelocityShear:
    """The LLSD of a volume: a plane fitted to the valid velocities of the window of every gate (``window``: a
    :class:`ShearWindow`, tables as ndarrays or tensors), its slope across the rays as azimuthal shear and along the ray as
    radial divergence, both in 1/s.  The fit of a gate is defined where its window holds at least ``min_valid`` valid gates and at
    least ``min_fraction`` of the full window (``floor(min_fraction * 65536 + 0.5)`` in 16-bit fixed point), the valid gates do not
    lie on one line, and, with ``centre_only``, the centre gate is valid.  ``want`` names the members to compute out of
    ``("azimuthal_shear", "radial_divergence", "velocity", "count")``; the others are ``None``.  One launch, no host
    synchronisation.  Returns :class:`VelocityShear`."""
    shape3 = _check_volume(vel, "vel")
    _check_size(vel, shape3)
    window = _check_window(window, shape3, wrap_rays)
    min_valid, q16, want = _check_fit(min_valid, min_fraction, want)
    _check_like(mask, vel, "mask", None)
    torch, lib, dev, src, m = _stage(vel, mask, [t for t in window[:2] if hasattr(t, "device")])
    tables = (_to_device(window.half_rays, dev), _to_device(window.az_scale, dev))
    with torch.cuda.device(dev):
        outs = _llsd(lib, torch, src, m, shape3, window, tables, wrap_rays, min_valid, q16, centre_only, want)
    shape = tuple(vel.shape)
    return VelocityShear(*(None if o is None else o.reshape(shape) for o in outs))


def azimuthal_shear_device(vel, window, *, median: Optional[Tuple[int, int]] = (1, 1), mask=None, wrap_rays: bool = True,
                           min_valid: int = 6, min_fraction: float = 0.5, centre_only: bool = False,
                           want=("azimuthal_shear", "radial_divergence")) -> VelocityShear:
    """The usual chain: the median filter of ``median = (half_rays, half_gates)`` rays and gates (``min_valid=1``,
    ``centre_only=True``: outliers go, holes stay), then the LLSD of its output.  ``mask`` applies to the median filter; what it
    leaves out is NaN for the LLSD.  ``median=None`` skips the filter.  Exactly :func:`median_filter_device` followed by
    :func:`velocity_shear_device`.  Returns :class:`VelocityShear`."""
    shape3 = _check_volume(vel, "vel")
    _check_size(vel, shape3)
    window = _check_window(window, shape3, wrap_rays)
    min_valid, q16, want = _check_fit(min_valid, min_fraction, want)
    _check_like(mask, vel, "mask", None)
    if median is not None:
        if not isinstance(median, (tuple, list)) or len(median) != 2:
            raise ValueError(f"median must be (half_rays, half_gates) or None, not {median!r}")
        median = _check_median(shape3, median[0], median[1], wrap_rays, 1)
    torch, lib, dev, src, m = _stage(vel, mask, [t for t in window[:2] if hasattr(t, "device")])
    tables = (_to_device(window.half_rays, dev), _to_device(window.az_scale, dev))
    with torch.cuda.device(dev):
        if median is not None:
            src, m = _median(lib, torch, src, m, shape3, median[0], median[1], wrap_rays, 1, True), None
        outs = _llsd(lib, torch, src, m, shape3, window, tables, wrap_rays, min_valid, q16, centre_only, want)
    shape = tuple(vel.shape)
    return VelocityShear(*(None if o is None else o.reshape(shape) for o in outs))


def velocity_shear(vel, window, **kw) -> VelocityShear:
    """:func:`azimuthal_shear_device` for NumPy arrays: the volume is staged through device memory and the members asked for
    come back as ndarrays."""
    r = azimuthal_shear_device(vel, window, **kw)
    return VelocityShear(*(None if o is None else o.cpu().numpy() for o in r))
