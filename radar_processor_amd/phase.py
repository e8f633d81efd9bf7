"""Differential phase in the polar domain, on the device (include/radargrid_phase.h; kernels in csrc/rg_phase.hip): what a
dual-polarisation volume needs BEFORE it is gridded.

* :func:`unfold_phidp_device` removes the +-wrap folds of PHIDP along every ray (Itoh's unwrapping);
* :func:`fit_phidp_device` fits a windowed least-squares line through it: the smoothed PHIDP and KDP (deg/km, one way);
* :func:`correct_attenuation_device` adds the path-integrated attenuation ``alpha * dPHIDP`` to Z and ``beta * dPHIDP`` to ZDR,
  along a path that never decreases;
* :func:`process_phase_device` chains the three; :func:`process_phase` is its NumPy-in, NumPy-out form.

Fields are float32 ``[n_rays, n_gates]`` (tensor or ndarray): one row is one ray, the sweeps of a volume are stacked, rays never
interact.  The outputs have the same shape; flattened they are what ``fields`` / ``masks`` of the gridders take.

The limit of the unfolding: a noise excursion beyond ``wrap / 2`` between neighbouring valid gates is taken for a fold and
shifts the rest of the ray, so mask the gates of low RHOHV (:func:`~radar_processor_amd.gate_filters.device_gate_mask`) first.

The contract is this build's own (the header states it; ``tests/phase_oracle.py`` restates it in NumPy and the tests hold the
kernels EQUAL to that, bit for bit: the sums are integers in 2^-16 degree fixed point).  Parity with PyART / wradlib is
unpinned.  Out of scope: ZPHI / self-consistent attenuation, R(KDP) and R(A), removal of the backscatter phase, Doppler
dealiasing.  The device functions enqueue on torch's current stream, validate every argument before the device is touched and
never synchronise with the host.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _native
from .convection import _finite
from .motion import _device_of, _dtype_name, _is_int, _to_device

MAX_GATES = _native.RG_PHASE_MAX_GATES
MAX_CLASSES = _native.RG_PHASE_MAX_CLASSES
MAX_HALF_WINDOW = _native.RG_PHASE_MAX_HALF_WINDOW
MAX_WORKGROUPS = _native.RG_PHASE_MAX_WORKGROUPS

#: ``band -> (alpha, beta)`` in dB per degree of PHIDP: ``A_H = alpha * KDP`` and ``A_DP = beta * KDP``.  S and X: Bringi,
#: Chandrasekar, Balakrishnan and Zrnic 1990 (J. Atmos. Oceanic Technol. 7, 829-840), as Bringi and Chandrasekar 2001 tabulate
#: them; C: Carey, Rutledge, Ahijevych and Keenan 2000 (J. Appl. Meteor. 39, 1405-1433).  Presets from the literature, not a
#: claim of parity with any package: both coefficients vary with temperature and drop shape by a factor of about two.
ATTENUATION_COEFFICIENTS = {"S": (0.017, 0.003), "C": (0.08, 0.02), "X": (0.25, 0.035)}


class PhaseFit(NamedTuple):
    """What :func:`fit_phidp_device` returns, each of the field's shape: ``kdp`` float32 deg/km (one way), ``phidp`` float32
    degrees (the fitted line at the gate), ``count`` uint16 (valid gates in the window); NaN where the fit is not defined."""
    kdp: object
    phidp: object
    count: object


class AttenuationCorrection(NamedTuple):
    """What :func:`correct_attenuation_device` returns: ``dbz`` and ``zdr`` corrected (``zdr`` None without a ZDR field),
    ``pia`` the dB added to Z, ``dphi`` the monotone PHIDP path in degrees."""
    dbz: object
    zdr: object
    pia: object
    dphi: object


class PhaseProducts(NamedTuple):
    """What :func:`process_phase_device` returns: ``phidp_unfolded``, ``phidp`` (smoothed), ``kdp``, ``count``, and the four
    members of :class:`AttenuationCorrection`."""
    phidp_unfolded: object
    phidp: object
    kdp: object
    count: object
    dbz: object
    zdr: object
    pia: object
    dphi: object


# ---- validation (host only) --------------------------------------------------------------------------------------------------
def _check_rays(field, what: str) -> Tuple[int, int]:
    if not hasattr(field, "shape") or not hasattr(field, "dtype"):
        raise ValueError(f"{what} must be a tensor or an ndarray, not {type(field).__name__}")
    shape = tuple(int(n) for n in field.shape)
    if _dtype_name(field) != "float32" or len(shape) != 2:
        raise ValueError(f"{what} must be float32 [n_rays, n_gates]; got {_dtype_name(field)} {list(shape)}")
    if shape[0] < 1 or shape[1] > MAX_GATES or shape[0] * shape[1] >= 2 ** 31:
        raise ValueError(f"{what}: at least one ray, at most {MAX_GATES} gates per ray and fewer than 2^31 gates in all; got "
                         f"{list(shape)}")
    if -(-shape[0] // 4) > MAX_WORKGROUPS:
        raise ValueError(f"{what}: at most {4 * MAX_WORKGROUPS} rays per call, got {shape[0]}: split the volume by rays")
    return shape


def _check_fit_rays(shape, what: str) -> None:
    """The fit takes one workgroup per ray and 512 gates, and one launch holds ``MAX_WORKGROUPS`` of them."""
    if shape[0] * -(-shape[1] // 512) > MAX_WORKGROUPS:
        raise ValueError(f"{what}: {shape[0]} rays of {shape[1]} gates are more than one fit takes ({MAX_WORKGROUPS} rays per 512 "
                         "gates): split the volume by rays")


def _check_like(other, field, what: str, dtype: Optional[str] = "float32") -> None:
    """``other`` (optional) has the shape of ``field`` and, unless ``dtype`` is None, that dtype."""
    if other is None:
        return
    if not hasattr(other, "shape") or tuple(int(n) for n in other.shape) != tuple(int(n) for n in field.shape):
        raise ValueError(f"{what} of shape {list(getattr(other, 'shape', []))} for a field of shape {list(field.shape)}")
    if dtype is not None and _dtype_name(other) != dtype:
        raise ValueError(f"{what} must be {dtype}, got {_dtype_name(other)}")


def _check_wrap(wrap) -> float:
    wrap = _finite(wrap, "wrap")
    with np.errstate(over="ignore"):
        half = float(np.float32(0.5 * wrap))
    if not (wrap > 0.0 and math.isfinite(half) and half > 0.0):
        raise ValueError(f"wrap must be positive with a finite positive float32 half, not {wrap!r}")
    return wrap


def _check_windows(half_window, dbz_edges, min_valid) -> Tuple[Tuple[int, ...], Tuple[float, ...], int]:
    try:
        edges = tuple(_finite(e, "dbz_edges: every edge") for e in dbz_edges)
    except TypeError:
        raise ValueError(f"dbz_edges must be a sequence of numbers, not {dbz_edges!r}") from None
    if any(b < a for a, b in zip(edges, edges[1:])):
        raise ValueError(f"dbz_edges must ascend, got {edges!r}")
    n_classes = len(edges) + 1
    if n_classes > MAX_CLASSES:
        raise ValueError(f"dbz_edges: at most {MAX_CLASSES - 1} edges ({MAX_CLASSES} classes), got {len(edges)}")
    if _is_int(half_window):
        half = (int(half_window),) * n_classes
    else:
        try:
            half = tuple(half_window)
        except TypeError:
            raise ValueError(f"half_window must be an integer or a sequence of integers, not {half_window!r}") from None
        if len(half) != n_classes or not all(_is_int(v) for v in half):
            raise ValueError(f"half_window: one integer per class ({n_classes} for {len(edges)} dbz_edges), got {half_window!r}")
        half = tuple(int(v) for v in half)
    if not all(1 <= v <= MAX_HALF_WINDOW for v in half):
        raise ValueError(f"half_window must lie in 1 .. {MAX_HALF_WINDOW}, got {half_window!r}")
    if not _is_int(min_valid) or not 2 <= min_valid <= 2 * MAX_HALF_WINDOW + 1:
        raise ValueError(f"min_valid must be an integer in 2 .. {2 * MAX_HALF_WINDOW + 1}, not {min_valid!r}")
    return half, edges, int(min_valid)


def _check_spacing(gate_spacing_m) -> float:
    spacing = _finite(gate_spacing_m, "gate_spacing_m")
    if spacing <= 0.0:
        raise ValueError(f"gate_spacing_m must be positive, got {gate_spacing_m!r}")
    return spacing


def _check_coefficients(alpha, beta, max_dphi) -> Tuple[float, float, float]:
    alpha, beta, max_dphi = _finite(alpha, "alpha"), _finite(beta, "beta"), _finite(max_dphi, "max_dphi")
    if alpha < 0.0 or beta < 0.0:
        raise ValueError(f"alpha and beta must not be negative, got {alpha!r} and {beta!r}")
    with np.errstate(over="ignore"):
        if not float(np.float32(max_dphi)) > 0.0:
            raise ValueError(f"max_dphi must be positive in float32, got {max_dphi!r}")
    return alpha, beta, max_dphi


def _check_band(band, alpha, beta) -> Tuple[float, float]:
    if band not in ATTENUATION_COEFFICIENTS:
        raise ValueError(f"band must be one of {sorted(ATTENUATION_COEFFICIENTS)}, not {band!r}")
    preset = ATTENUATION_COEFFICIENTS[band]
    return (preset[0] if alpha is None else alpha), (preset[1] if beta is None else beta)


def scale_for(gate_spacing_m: float) -> float:
    """The ``scale`` of ``rg_phidp_fit_f32`` that makes KDP one-way deg/km: ``500 / (65536 * gate_spacing_m)`` -- half the
    slope of the two-way PHIDP per metre, times 1000, over the 2^16 of the fixed point."""
    return 500.0 / (65536.0 * gate_spacing_m)


# ---- device ------------------------------------------------------------------------------------------------------------------
def _unfold(lib, torch, src, m, shape, wrap, want_folds):
    out = torch.empty(shape, dtype=torch.float32, device=src.device)
    folds = torch.empty(shape, dtype=torch.int32, device=src.device) if want_folds else None
    if shape[1]:                 # rays without gates: the empty outputs are the result (and an empty tensor has no address)
        _native.check(lib.rg_phidp_unfold_f32(_native.ptr(src), _native.ptr(m), shape[0], shape[1], wrap, _native.ptr(out),
                                              _native.ptr(folds), _native.stream_ptr()), "rg_phidp_unfold_f32")
    return out, folds


def _fit(lib, torch, phi, z, shape, half, edges, min_valid, centre_only, scale):
    kdp = torch.empty(shape, dtype=torch.float32, device=phi.device)
    smooth = torch.empty(shape, dtype=torch.float32, device=phi.device)
    count = torch.empty(shape, dtype=torch.uint16, device=phi.device)
    c_edges = (_native.c_double * max(len(edges), 1))(*edges)
    c_half = (_native.c_int32 * len(half))(*half)
    if shape[1]:
        _native.check(lib.rg_phidp_fit_f32(_native.ptr(phi), shape[0], shape[1], _native.ptr(z), c_edges, c_half, len(half), min_valid,
                                           1 if centre_only else 0, scale, _native.ptr(kdp), _native.ptr(smooth), _native.ptr(count),
                                           _native.stream_ptr()), "rg_phidp_fit_f32")
    return PhaseFit(kdp, smooth, count)


def _attenuation(lib, torch, smooth, origin, z, zd, shape, alpha, beta, max_dphi):
    out = torch.empty(shape, dtype=torch.float32, device=smooth.device)
    zout = None if zd is None else torch.empty(shape, dtype=torch.float32, device=smooth.device)
    pia = torch.empty(shape, dtype=torch.float32, device=smooth.device)
    dphi = torch.empty(shape, dtype=torch.float32, device=smooth.device)
    if shape[1]:
        _native.check(lib.rg_attenuation_phidp_f32(_native.ptr(smooth), _native.ptr(origin), shape[0], shape[1], alpha, beta, max_dphi,
                                                   _native.ptr(z), _native.ptr(zd), _native.ptr(out), _native.ptr(zout),
                                                   _native.ptr(pia), _native.ptr(dphi), _native.stream_ptr()),
                      "rg_attenuation_phidp_f32")
    return AttenuationCorrection(out, zout, pia, dphi)


def _check_phi0(phi0, n_rays):
    """None, or a float32 ``[n_rays]`` array / tensor; a number becomes that array."""
    if phi0 is None:
        return None
    if not hasattr(phi0, "shape"):
        return np.full(n_rays, _finite(phi0, "phi0"), np.float32)
    if tuple(int(n) for n in phi0.shape) != (n_rays,) or _dtype_name(phi0) != "float32":
        raise ValueError(f"phi0 must be a number or float32 [{n_rays}], got {_dtype_name(phi0)} {list(phi0.shape)}")
    return phi0


def unfold_phidp_device(phidp, *, mask=None, wrap: float = 360.0, return_folds: bool = False):
    """PHIDP (float32 ``[n_rays, n_gates]`` degrees) without its folds, as float32 of the same shape on the device: along every
    ray a step of more than ``wrap / 2`` between one valid gate and the previous valid gate, however far back, counts as a
    fold, and ``wrap`` times the running fold count is added.  A gate is valid when it is finite and ``mask`` (optional, any
    integer or bool type; non-zero leaves the gate out) is 0 there; the other gates come out NaN.  ``return_folds=True`` also
    returns the int32 fold count (0 at invalid gates).  A noise excursion beyond ``wrap / 2`` shifts the rest of its ray: mask
    low RHOHV first."""
    shape = _check_rays(phidp, "phidp")
    _check_like(mask, phidp, "mask", None)
    wrap = _check_wrap(wrap)
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(phidp, mask)
    src = _to_device(phidp, dev)
    m = None if mask is None else _to_device(mask, dev, torch.uint8)
    with torch.cuda.device(dev):
        out, folds = _unfold(lib, torch, src, m, shape, wrap, return_folds)
    return (out, folds) if return_folds else out


def fit_phidp_device(phidp, gate_spacing_m, *, half_window=15, min_valid: int = 8, dbz=None, dbz_edges: Sequence[float] = (),
                     centre_only: bool = False) -> PhaseFit:
    """A least-squares line through the unfolded ``phidp`` in the window of ``half_window`` gates on either side of every
    gate: :class:`PhaseFit` with KDP (half the slope, deg/km one way), the line's value at the gate and the number of valid
    gates in the window.  The fit is defined where at least ``min_valid`` gates of the window are valid (finite, at most 16384
    degrees in magnitude) and lie at two positions or more; ``centre_only=True`` also requires the gate itself, otherwise gaps
    inside an echo are filled.  ``dbz`` with ``dbz_edges`` (up to three ascending dBZ values) picks the window per gate:
    ``half_window`` is then a sequence with one entry per class, class k = the number of edges at or below the gate's dBZ (NaN:
    class 0) -- long windows in weak echo, short ones in cores."""
    shape = _check_rays(phidp, "phidp")
    _check_fit_rays(shape, "phidp")
    spacing = _check_spacing(gate_spacing_m)
    half, edges, min_valid = _check_windows(half_window, dbz_edges, min_valid)
    _check_like(dbz, phidp, "dbz")
    if edges and dbz is None:
        raise ValueError("dbz_edges without dbz: the classes are chosen by reflectivity")
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(phidp, dbz)
    phi = _to_device(phidp, dev)
    z = None if dbz is None else _to_device(dbz, dev)
    with torch.cuda.device(dev):
        return _fit(lib, torch, phi, z, shape, half, edges, min_valid, centre_only, scale_for(spacing))


def correct_attenuation_device(phidp_smooth, dbz, *, zdr=None, alpha: float, beta: float, phi0=None,
                               max_dphi: float = 360.0) -> AttenuationCorrection:
    """Z and ZDR corrected for attenuation along the ray by the linear-PHIDP method: with ``dphi`` the running maximum of
    ``phidp_smooth - origin``, clamped to ``0 .. max_dphi`` degrees, ``dbz + alpha * dphi`` and ``zdr + beta * dphi``
    (``alpha``, ``beta`` in dB per degree: :data:`ATTENUATION_COEFFICIENTS`).  The origin of a ray is ``phi0`` (a number, or
    float32 ``[n_rays]``; NaN entries fall back) or its first non-NaN ``phidp_smooth``.  The path never decreases, so noise and
    a falling PHIDP (backscatter phase) never take attenuation back; NaN gates of ``phidp_smooth`` keep the value reached before
    them.  A NaN ``dbz`` stays NaN."""
    shape = _check_rays(phidp_smooth, "phidp_smooth")
    _check_like(dbz, phidp_smooth, "dbz")
    if dbz is None:
        raise ValueError("dbz is required")
    _check_like(zdr, phidp_smooth, "zdr")
    alpha, beta, max_dphi = _check_coefficients(alpha, beta, max_dphi)
    phi0 = _check_phi0(phi0, shape[0])
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(phidp_smooth, dbz, zdr)
    smooth, z = _to_device(phidp_smooth, dev), _to_device(dbz, dev)
    zd = None if zdr is None else _to_device(zdr, dev)
    origin = None if phi0 is None else _to_device(phi0, dev)
    with torch.cuda.device(dev):
        return _attenuation(lib, torch, smooth, origin, z, zd, shape, alpha, beta, max_dphi)


def process_phase_device(phidp, dbz, gate_spacing_m, *, zdr=None, mask=None, band: str = "C", alpha=None, beta=None,
                         wrap: float = 360.0, half_window=15, min_valid: int = 8, dbz_edges: Sequence[float] = (),
                         centre_only: bool = False, phi0=None, max_dphi: float = 360.0) -> PhaseProducts:
    """The chain on one volume: unfold ``phidp`` under ``mask``, fit it (windows chosen by ``dbz`` when ``dbz_edges`` are
    given), correct ``dbz`` and ``zdr`` with the coefficients of ``band`` (``alpha`` / ``beta`` override them).  Three launches
    on the current stream, nothing returns to the host.  Returns :class:`PhaseProducts`."""
    shape = _check_rays(phidp, "phidp")
    _check_fit_rays(shape, "phidp")
    _check_like(dbz, phidp, "dbz")
    if dbz is None:
        raise ValueError("dbz is required")
    _check_like(zdr, phidp, "zdr")
    _check_like(mask, phidp, "mask", None)
    spacing = _check_spacing(gate_spacing_m)
    wrap = _check_wrap(wrap)
    half, edges, min_valid = _check_windows(half_window, dbz_edges, min_valid)
    alpha, beta, max_dphi = _check_coefficients(*_check_band(band, alpha, beta), max_dphi)
    phi0 = _check_phi0(phi0, shape[0])
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(phidp, dbz, zdr, mask)
    src, z = _to_device(phidp, dev), _to_device(dbz, dev)
    zd = None if zdr is None else _to_device(zdr, dev)
    m = None if mask is None else _to_device(mask, dev, torch.uint8)
    origin = None if phi0 is None else _to_device(phi0, dev)
    with torch.cuda.device(dev):
        unfolded, _ = _unfold(lib, torch, src, m, shape, wrap, False)
        fit = _fit(lib, torch, unfolded, z if edges else None, shape, half, edges, min_valid, centre_only, scale_for(spacing))
        corr = _attenuation(lib, torch, fit.phidp, origin, z, zd, shape, alpha, beta, max_dphi)
    return PhaseProducts(unfolded, fit.phidp, fit.kdp, fit.count, corr.dbz, corr.zdr, corr.pia, corr.dphi)


def process_phase(phidp, dbz, gate_spacing_m, **kw) -> PhaseProducts:
    """:func:`process_phase_device` for NumPy arrays: the fields are staged through device memory and every member of the
    :class:`PhaseProducts` comes back as an ndarray (``count`` as uint16)."""
    result = process_phase_device(phidp, dbz, gate_spacing_m, **kw)
    return PhaseProducts(*(None if r is None else r.cpu().numpy() for r in result))
