"""Convective and stratiform rain on the device after Steiner, Houze and Yuter 1995 (include/radargrid_hip.h, "Convective /
stratiform classification"; kernels in csrc/rg_convection.hip): which echo is a convective core and which is not.

* :func:`disk_footprint` turns a radius in metres into the half-width table of the C ABI (host, float64);
* :func:`echo_background_device` is the background reflectivity -- the mean of LINEAR reflectivity over a disk, in dBZ --
  a product in its own right (``rg_echo_table_f32``, ``rg_disk_background``);
* :func:`convective_stratiform_device` classifies planes: 0 no echo, 1 stratiform, 2 convective
  (plus ``rg_convective_centres_f32``, ``rg_convective_area_u8``); :func:`convective_stratiform` is its NumPy-in, NumPy-out
  wrapper and :func:`classify_grid` takes the CAPPI of the work level from a stored grid first;
* :func:`rain_rate_by_class_device` applies one ``Z = a R^b`` to the stratiform and another to the convective pixels.

Definitions (the header's): a pixel has ECHO when it is not NaN, its mask is 0 and ``dBZ >= min_dbz`` in float32.  The
background of a pixel is ``10 log10`` of the mean linear reflectivity of the echo pixels within ``background_radius`` of it
(NaN where there is none).  An echo pixel is a convective CENTRE when ``dBZ >= intense`` or when it exceeds its background by
``delta(bkg)`` -- ``peak_a`` below 0 dBZ, ``max(peak_a - bkg^2 / peak_b, 0)`` above.  Every centre makes the echo pixels
within a radius convective; the radius grows with the centre's background through ``area_relation``.

The relations are those of Steiner et al. 1995 as PyART's ``steiner_conv_strat`` carries them; parity with PyART unpinned.
Linear reflectivity is summed in 2^-16 fixed point, so every sum is an integer and the results are bit-reproducible: the tests
hold them equal to a NumPy restatement (``tests/convection_oracle.py``).  The device functions take tensors or ndarrays,
enqueue on torch's current stream, validate every argument before the device is touched and never synchronise with the host.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import numpy as np

from . import _native
from .accumulation import _check_zr, rain_rate_device
from .components import _axes
from .motion import _check_mask, _check_planes, _device_of, _is_tensor, _to_device

MAX_RADIUS = _native.RG_MAX_DISK_RADIUS
MAX_CLASSES = _native.RG_MAX_CONV_CLASSES
PEAK_RELATIONS = {"steiner": (10.0, 180.0)}
_KM = (1000.0, 2000.0, 3000.0, 4000.0, 5000.0)
AREA_RELATIONS = {"small": ((30.0, 35.0, 40.0, 45.0), _KM), "medium": ((25.0, 30.0, 35.0, 40.0), _KM),
                  "large": ((20.0, 25.0, 30.0, 35.0), _KM)}
_CLASSIFY_KEYS = ("min_dbz", "intense", "peak_relation", "area_relation", "background_radius")


class ConvectiveStratiform(NamedTuple):
    """What :func:`convective_stratiform_device` returns with ``return_parts=True``, everything of the planes' shape:
    ``classes`` uint8 (0 no echo, 1 stratiform, 2 convective), ``background`` float32 dBZ (NaN without echo in reach),
    ``centres`` uint8 (0, or the radius class 1 .. K of the convective centre at the pixel)."""
    classes: object
    background: object
    centres: object


# ---- validation (host only) --------------------------------------------------------------------------------------------------
def _finite(value, what: str) -> float:
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a number, not {value!r}") from None
    if not math.isfinite(value):
        raise ValueError(f"{what} must be finite, not {value!r}")
    return value


def _check_min_dbz(min_dbz) -> float:
    value = _finite(min_dbz, "min_dbz")
    with np.errstate(over="ignore"):
        value32 = float(np.float32(value))
    if not math.isfinite(value32):
        raise ValueError(f"min_dbz must be a finite float32 value, not {min_dbz!r}")
    return value32


def disk_footprint(radius_m, dy, dx) -> Tuple[int, ...]:
    """The half-widths ``hw[0 .. ry]`` of the disk of ``radius_m`` metres on a grid of ``dy`` x ``dx`` metres, in float64 on
    the host: ``ry`` is the largest ``d`` with ``(d * dy)^2 <= R^2`` and ``hw[d]`` the largest ``k >= 0`` with
    ``(k * dx)^2 <= R^2 - (d * dy)^2`` -- the pixel ``(dy', dx')`` belongs iff its centre lies within ``R`` of the middle.
    ``ValueError`` for a radius of more than 127 pixels along either axis."""
    R, dy, dx = _finite(radius_m, "radius_m"), _finite(dy, "dy"), _finite(dx, "dx")
    if R < 0.0 or dy <= 0.0 or dx <= 0.0:
        raise ValueError(f"disk_footprint needs radius_m >= 0 and dy, dx > 0, got {radius_m!r}, {dy!r} and {dx!r}")
    if R / dy >= MAX_RADIUS + 1 or R / dx >= MAX_RADIUS + 1:
        raise ValueError(f"a radius of {R!r} m is {R / dy:.1f} x {R / dx:.1f} pixels at dy={dy!r} m and dx={dx!r} m: more than "
                         f"{MAX_RADIUS}; it fits at a spacing above {R / (MAX_RADIUS + 1):.6g} m")

    def largest(step, limit):                    # the largest k >= 0 with (k * step)^2 <= limit, limit >= 0
        k = int(math.sqrt(limit) / step)
        while (k + 1) * step * ((k + 1) * step) <= limit:
            k += 1
        while k > 0 and k * step * (k * step) > limit:
            k -= 1
        return k

    ry = largest(dy, R * R)
    return tuple(largest(dx, R * R - (d * dy) * (d * dy)) for d in range(ry + 1))


def _check_peak(peak_relation) -> Tuple[float, float]:
    if isinstance(peak_relation, str):
        if peak_relation not in PEAK_RELATIONS:
            raise ValueError(f"peak_relation must be one of {sorted(PEAK_RELATIONS)} or an (a, b) pair, not {peak_relation!r}")
        return PEAK_RELATIONS[peak_relation]
    try:
        a, b = peak_relation
    except (TypeError, ValueError):
        raise ValueError(f"peak_relation must be one of {sorted(PEAK_RELATIONS)} or an (a, b) pair, not {peak_relation!r}") from None
    a, b = _finite(a, "peak_relation a"), _finite(b, "peak_relation b")
    if b <= 0.0:
        raise ValueError(f"peak_relation: b must be positive, got {b!r}")
    return a, b


def _check_area(area_relation) -> Tuple[Tuple[float, ...], Tuple[float, ...]]:
    """``(edges, radii_m)``: K - 1 ascending finite edges in dBZ and K radii in metres, K in 1 .. 8."""
    if isinstance(area_relation, str):
        if area_relation not in AREA_RELATIONS:
            raise ValueError(f"area_relation must be one of {sorted(AREA_RELATIONS)} or (edges, radii_m), not {area_relation!r}")
        return AREA_RELATIONS[area_relation]
    try:
        edges, radii = area_relation
        edges, radii = tuple(edges), tuple(radii)
    except (TypeError, ValueError):
        raise ValueError(f"area_relation must be one of {sorted(AREA_RELATIONS)} or (edges, radii_m), not {area_relation!r}") from None
    if not 1 <= len(radii) <= MAX_CLASSES or len(edges) != len(radii) - 1:
        raise ValueError(f"area_relation: 1 .. {MAX_CLASSES} radii and one edge fewer, got {len(radii)} radii and {len(edges)} edges")
    edges = tuple(_finite(e, "area_relation: every edge") for e in edges)
    radii = tuple(_finite(r, "area_relation: every radius") for r in radii)
    if any(b < a for a, b in zip(edges, edges[1:])):
        raise ValueError(f"area_relation: the edges must ascend, got {edges!r}")
    if any(r < 0.0 for r in radii):
        raise ValueError(f"area_relation: the radii must not be negative, got {radii!r}")
    return edges, radii


def _check_spacing(dx, dy, geometry, h, w) -> Tuple[float, float]:
    """``(dy, dx)`` in metres from ``geometry`` (anything with ``grid_shape`` / ``grid_limits``, as in
    :func:`~radar_processor_amd.components.cell_table_device`) or from ``dx`` / ``dy`` (``dy`` defaults to ``dx``)."""
    if geometry is not None:
        if dx is not None or dy is not None:
            raise ValueError("give the spacing through geometry or through dx / dy, not both")
        _, step_y, _, step_x = _axes(geometry, h, w)
        dy, dx = abs(step_y), abs(step_x)
        dy, dx = dy or dx, dx or dy                      # a single row or column has no step of its own: the other axis'
    elif dx is None:
        raise ValueError("the pixel spacing is required: dx (and dy) in metres, or geometry")
    dx = _finite(dx, "dx")
    dy = dx if dy is None else _finite(dy, "dy")
    if dx <= 0.0 or dy <= 0.0:
        raise ValueError(f"the pixel spacing must be positive, got dy={dy!r} and dx={dx!r}")
    return dy, dx


# ---- device ------------------------------------------------------------------------------------------------------------------
def _c_footprint(hw):
    return (_native.c_int32 * len(hw))(*hw)


def _echo_table(lib, torch, src, m, shape3, min_dbz):
    need = int(lib.rg_echo_table_bytes(*shape3))
    if need < 0:
        _native.check(need, "rg_echo_table_bytes")
    table = torch.empty(max(need, 16), dtype=torch.uint8, device=src.device)
    _native.check(lib.rg_echo_table_f32(_native.ptr(src), _native.ptr(m), *shape3, min_dbz, _native.ptr(table), need,
                                        _native.stream_ptr()), "rg_echo_table_f32")
    return table


def _background(lib, torch, src, m, shape3, min_dbz, hw, want_counts=False):
    table = _echo_table(lib, torch, src, m, shape3, min_dbz)
    bkg = torch.empty(shape3, dtype=torch.float32, device=src.device)
    count = torch.empty(shape3, dtype=torch.int32, device=src.device) if want_counts else None
    _native.check(lib.rg_disk_background(_native.ptr(table), *shape3, _c_footprint(hw), len(hw) - 1, 0, _native.ptr(count),
                                         _native.ptr(bkg), _native.stream_ptr()), "rg_disk_background")
    return bkg, count


def _centres(lib, torch, src, m, bkg, shape3, min_dbz, intense, peak, edges):
    out = torch.empty(shape3, dtype=torch.uint8, device=src.device)
    c_edges = (_native.c_double * max(len(edges), 1))(*edges)
    _native.check(lib.rg_convective_centres_f32(_native.ptr(src), _native.ptr(m), _native.ptr(bkg), *shape3, min_dbz, intense,
                                                peak[0], peak[1], c_edges, len(edges) + 1, _native.ptr(out), _native.stream_ptr()),
                  "rg_convective_centres_f32")
    return out


def _area(lib, torch, centres, src, m, shape3, min_dbz, footprints):
    K = len(footprints)
    need = int(lib.rg_convective_area_workspace_bytes(*shape3, K))
    if need < 0:
        _native.check(need, "rg_convective_area_workspace_bytes")
    workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=src.device)
    out = torch.empty(shape3, dtype=torch.uint8, device=src.device)
    rows = (_native.c_int32 * (K * (MAX_RADIUS + 1)))()
    for k, hw in enumerate(footprints):
        rows[k * (MAX_RADIUS + 1):k * (MAX_RADIUS + 1) + len(hw)] = hw
    ry = (_native.c_int32 * K)(*[len(hw) - 1 for hw in footprints])
    _native.check(lib.rg_convective_area_u8(_native.ptr(centres), _native.ptr(src), _native.ptr(m), *shape3, min_dbz, K, rows, ry,
                                            _native.ptr(workspace), need, _native.ptr(out), _native.stream_ptr()),
                  "rg_convective_area_u8")
    return out


def _stage(planes, mask):
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(planes, mask)
    src = _to_device(planes, dev)
    m = None if mask is None else _to_device(mask, dev, torch.uint8)
    return torch, lib, dev, src, m


def _check_stack(planes, mask):
    shape3 = _check_planes(planes, "planes")
    if shape3[0] > 65535:
        raise ValueError(f"planes: at most 65535 planes per call, got {shape3[0]}")
    _check_mask(mask, planes, "mask")
    return shape3


def echo_background_device(planes, *, dx, dy=None, radius: float = 11000.0, min_dbz: float = 5.0, mask=None,
                           return_counts: bool = False):
    """The background reflectivity of dBZ ``planes`` (float32 ``[h, w]`` or ``[n, h, w]``): at every pixel, echo or not,
    ``10 log10`` of the mean LINEAR reflectivity of the echo pixels within ``radius`` metres, as float32 of the planes' shape;
    NaN where no echo lies in reach.  ``dx`` / ``dy``: the pixel spacing in metres (``dy`` defaults to ``dx``); ``mask``
    (optional): non-zero leaves the pixel out.  ``return_counts=True`` also returns the int32 number of echo pixels in the
    disk.  Values are clamped to -10 .. 80 dBZ before they are averaged.  :func:`disk_footprint` shapes the disk; a radius
    beyond 127 pixels is a ``ValueError``."""
    shape3 = _check_stack(planes, mask)
    dy, dx = _check_spacing(dx, dy, None, shape3[1], shape3[2])
    hw = disk_footprint(radius, dy, dx)
    min_dbz = _check_min_dbz(min_dbz)
    torch, lib, dev, src, m = _stage(planes, mask)
    with torch.cuda.device(dev):
        bkg, count = _background(lib, torch, src, m, shape3, min_dbz, hw, return_counts)
    shape = tuple(planes.shape)
    return (bkg.reshape(shape), count.reshape(shape)) if return_counts else bkg.reshape(shape)


def convective_stratiform_device(planes, *, dx=None, dy=None, geometry=None, mask=None, min_dbz: float = 5.0, intense: float = 40.0,
                                 peak_relation="steiner", area_relation="medium", background_radius: float = 11000.0,
                                 return_parts: bool = False):
    """Classify dBZ ``planes`` (float32 ``[h, w]`` or ``[n, h, w]``, tensor or ndarray) into uint8 of the same shape:
    0 no echo, 1 stratiform, 2 convective.

    The spacing comes from ``geometry`` (anything with ``grid_shape`` / ``grid_limits`` whose last two axes are the planes')
    or from ``dx`` / ``dy`` in metres.  ``mask`` (optional): non-zero leaves the pixel out.  ``min_dbz``: the echo threshold.
    ``intense``: at or above it a pixel is a centre whatever its surroundings.  ``peak_relation``: ``"steiner"``
    (``a, b = 10, 180``) or an ``(a, b)`` pair for ``delta = max(a - bkg^2 / b, 0)``.  ``area_relation``: ``"small"``,
    ``"medium"``, ``"large"`` or ``(edges, radii_m)`` -- K - 1 ascending background edges in dBZ and the K radii in metres of
    the convective area around a centre whose background lies below the first edge, between the edges, at or above the last
    one.  ``background_radius``: the radius of the background disk in metres.

    ``return_parts=True`` returns :class:`ConvectiveStratiform` with the background and the centre plane as well."""
    shape3 = _check_stack(planes, mask)
    dy, dx = _check_spacing(dx, dy, geometry, shape3[1], shape3[2])
    min_dbz, intense = _check_min_dbz(min_dbz), _finite(intense, "intense")
    peak = _check_peak(peak_relation)
    edges, radii = _check_area(area_relation)
    hw = disk_footprint(background_radius, dy, dx)
    footprints = [disk_footprint(r, dy, dx) for r in radii]
    torch, lib, dev, src, m = _stage(planes, mask)
    with torch.cuda.device(dev):
        bkg, _ = _background(lib, torch, src, m, shape3, min_dbz, hw)
        centres = _centres(lib, torch, src, m, bkg, shape3, min_dbz, intense, peak, edges)
        classes = _area(lib, torch, centres, src, m, shape3, min_dbz, footprints)
    shape = tuple(planes.shape)
    if return_parts:
        return ConvectiveStratiform(classes.reshape(shape), bkg.reshape(shape), centres.reshape(shape))
    return classes.reshape(shape)


def convective_stratiform(planes, **kw):
    """:func:`convective_stratiform_device` for NumPy arrays: the uint8 classes, or a :class:`ConvectiveStratiform` of arrays
    with ``return_parts=True``."""
    result = convective_stratiform_device(planes, **kw)
    if isinstance(result, ConvectiveStratiform):
        return ConvectiveStratiform(*(r.cpu().numpy() for r in result))
    return result.cpu().numpy()


def classify_grid(grid, geometry, altitude: float = 3000.0, **kw):
    """Classify a stored grid ``[nz, ny, nx]`` at its work level: the CAPPI at ``altitude`` metres
    (:func:`~radar_processor_amd.grid_products.constant_altitude_ppi`), then :func:`convective_stratiform_device` with the
    spacing of ``geometry``; further keywords go to it.  Returns what it returns, on the device."""
    if "dx" in kw or "dy" in kw or "geometry" in kw:
        raise ValueError("classify_grid takes the spacing from its geometry: pass no dx, dy or geometry keyword")
    from .grid_products import constant_altitude_ppi
    plane = constant_altitude_ppi(grid, geometry, altitude)
    if not _is_tensor(plane):
        plane = np.ascontiguousarray(np.ma.getdata(plane), dtype=np.float32)
    return convective_stratiform_device(plane, geometry=geometry, **kw)


def rain_rate_by_class_device(planes, classes, *, stratiform=(200.0, 1.6), convective=(300.0, 1.4), min_dbz: float = 5.0,
                              max_dbz: float = 55.0, mask=None):
    """mm/h of dBZ ``planes`` under two relations ``Z = a R^b``: ``convective = (a, b)`` where ``classes`` (uint8 of the
    planes' shape, from :func:`convective_stratiform_device`) is 2, ``stratiform = (a, b)`` everywhere else.  Two
    :func:`~radar_processor_amd.accumulation.rain_rate_device` planes and one selection on the device; NaN, 0 and the
    ``max_dbz`` cap are that function's."""
    _check_planes(planes, "planes")
    if not hasattr(classes, "shape") or tuple(int(v) for v in classes.shape) != tuple(int(v) for v in planes.shape):
        raise ValueError(f"classes of shape {list(getattr(classes, 'shape', []))} for planes of shape {list(planes.shape)}")
    if str(classes.dtype).replace("torch.", "") != "uint8":
        raise ValueError(f"classes must be uint8, got {classes.dtype}")
    try:
        (sa, sb), (ca, cb) = stratiform, convective
    except (TypeError, ValueError):
        raise ValueError(f"stratiform and convective must be (a, b) pairs, got {stratiform!r} and {convective!r}") from None
    _check_zr(sa, sb, min_dbz, max_dbz)
    _check_zr(ca, cb, min_dbz, max_dbz)
    _check_mask(mask, planes, "mask")
    torch = _native.torch_mod()
    dev = _device_of(planes, classes, mask)
    src, cls = _to_device(planes, dev), _to_device(classes, dev)
    m = None if mask is None else _to_device(mask, dev, torch.uint8)
    calm = rain_rate_device(src, a=sa, b=sb, min_dbz=min_dbz, max_dbz=max_dbz, mask=m)
    heavy = rain_rate_device(src, a=ca, b=cb, min_dbz=min_dbz, max_dbz=max_dbz, mask=m)
    return torch.where(cls == 2, heavy, calm)


def _check_classify(classify: Optional[dict]) -> dict:
    """The keywords a :class:`~radar_processor_amd.accumulation.RainAccumulator` hands to the classification, validated on
    the host; ``dx`` (and ``dy``) or ``geometry`` are required among them."""
    classify = dict(classify or {})
    unknown = sorted(set(classify) - set(_CLASSIFY_KEYS) - {"dx", "dy", "geometry"})
    if unknown:
        raise ValueError(f"classify: unknown keyword(s) {unknown}: expected some of {list(_CLASSIFY_KEYS + ('dx', 'dy', 'geometry'))}")
    if classify.get("geometry") is None and classify.get("dx") is None:
        raise ValueError("classify must give the pixel spacing: dx (and dy) in metres, or geometry")
    if "min_dbz" in classify:
        _check_min_dbz(classify["min_dbz"])
    if "intense" in classify:
        _finite(classify["intense"], "intense")
    _check_peak(classify.get("peak_relation", "steiner"))
    _check_area(classify.get("area_relation", "medium"))
    _finite(classify.get("background_radius", 11000.0), "background_radius")
    return classify
