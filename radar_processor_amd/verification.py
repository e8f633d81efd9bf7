"""Nowcast verification on the device (include/radargrid_hip.h, "Nowcast verification"; kernels in csrc/rg_verify.hip): how
good a forecast plane is against the observation it was made for.

* :func:`contingency_device` counts hits, false alarms, misses and correct negatives at thresholds (``rg_contingency_f32``);
  :func:`categorical_scores` turns a :class:`ContingencyTable` into POD, FAR, CSI, bias, ETS, HSS and the base rate (host);
* :func:`exceedance_sat_device` builds the summed-area tables of the threshold exceedances (``rg_exceedance_sat_i32``);
* :func:`neighbourhood_fraction_device` is the product that falls out of them: the fraction of a neighbourhood at or above a
  threshold (``rg_box_fraction_f32``);
* :func:`fss_device` sums the three terms of the fractions skill score over a ladder of window sizes (``rg_fss_sums_i32``) and
  returns :class:`FSSSums`;
* :func:`verify_nowcast` does both for a stack of lead times in one call;
* :class:`NowcastVerifier` runs along a sequence of scans, verifies every advection nowcast of :mod:`.motion` AND the
  persistence forecast when their target frame arrives, and keeps the totals per lead -- what
  :class:`~radar_processor_amd.tracking.CellTracker` is for cells and
  :class:`~radar_processor_amd.accumulation.RainAccumulator` for rainfall.

Definitions (the header's): a pixel is VALID when neither field is NaN there and the mask is 0 (+-inf are values); it EXCEEDS
a threshold when it is valid and ``v >= t`` in float32 -- an invalid pixel exceeds nothing in either field.  The WINDOW of
scale ``n`` (1 .. 255) at ``(y, x)`` covers rows ``y - n // 2 .. y - n // 2 + n - 1`` and the same span of columns, cut to the
plane: ``scipy.ndimage.uniform_filter(size=n, mode="constant", cval=0) * n * n``.  That is also the convention of pysteps'
``fss`` (zero padding, non-finite counted as no exceedance, sums over all pixels); parity with pysteps unpinned.

Every sum is an integer, so the results are exact: the tests hold them equal to a NumPy restatement
(``tests/verification_oracle.py``).  The device functions take tensors or ndarrays, enqueue on torch's current stream,
validate every argument before the device is touched and never synchronise with the host.

MEMORY: the two tables are int32 ``[n, T, h, w]`` each -- 0.77 GB for 6 leads x 4 thresholds at 2000 x 2000.  There is no
chunking: verify fewer leads or thresholds per call where that does not fit.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import numpy as np

from . import _native
from .motion import (_ADVECT_KEYS, _ESTIMATE_KEYS, ADVECT_METHODS, MAX_LEADS, MAX_SUBSTEPS, MotionGrid, _check_blocks, _check_field,
                     _check_levels, _check_mask, _check_planes, _device_of, _is_int, _is_tensor, _to_device, advect_device,
                     estimate_motion_device, fill_motion_device)

MAX_THRESHOLDS = _native.RG_MAX_VERIFY_THRESHOLDS
MAX_SCALES = _native.RG_MAX_VERIFY_SCALES
MAX_SCALE = _native.RG_MAX_VERIFY_SCALE
_VERIFIER_ESTIMATE_KEYS = tuple(k for k in _ESTIMATE_KEYS if not k.startswith("mask_"))      # the masks come with the frames
_VERIFIER_ADVECT_KEYS = tuple(k for k in _ADVECT_KEYS if k in ("method", "substeps"))


class ContingencyTable(NamedTuple):
    """Counts per plane and threshold, int64 on the device: ``hits`` (both exceed), ``false_alarms`` (the forecast only),
    ``misses`` (the observation only), ``correct_negatives`` (neither, among the valid) ``[n, T]``; ``valid [n]`` the valid
    pixels.  ``a + b`` adds two tables of one shape exactly (more scans of the same leads and thresholds)."""
    hits: object
    false_alarms: object
    misses: object
    correct_negatives: object
    valid: object

    def __add__(self, other):
        if not isinstance(other, ContingencyTable):
            return NotImplemented
        if tuple(self.hits.shape) != tuple(other.hits.shape):
            raise ValueError(f"tables of {list(self.hits.shape)} and {list(other.hits.shape)} (planes, thresholds) do not add")
        return ContingencyTable(*(a + b for a, b in zip(self, other)))


class FSSSums(NamedTuple):
    """The integer sums of the fractions skill score, int64 on the device.  ``sums [n, T, S, 3]`` = ``(A, B, C)`` =
    ``(sum (cf - co)^2, sum cf^2, sum co^2)`` over ALL pixels, with ``cf`` / ``co`` the window counts of the forecast and the
    observation; ``observed [n, T]`` the observation's exceeding pixels and ``pixels [n]`` the pixels of a plane (the
    denominators of the base rate).  ``a + b`` adds two of one shape exactly: the FSS of the sum is the FSS aggregated over
    both scans."""
    sums: object
    observed: object
    pixels: object

    def __add__(self, other):
        if not isinstance(other, FSSSums):
            return NotImplemented
        if tuple(self.sums.shape) != tuple(other.sums.shape):
            raise ValueError(f"sums of {list(self.sums.shape)} and {list(other.sums.shape)} do not add")
        return FSSSums(*(a + b for a, b in zip(self, other)))

    def fss(self) -> np.ndarray:
        """float64 ``[n, T, S]`` on the host: ``1 - A / (B + C)``; NaN where ``B + C == 0`` (nothing exceeds in either
        field: the score says nothing).  Reads the sums back."""
        s = _host(self.sums)
        a, bc = s[..., 0].astype(np.float64), (s[..., 1] + s[..., 2]).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(bc > 0, 1.0 - a / bc, np.nan)

    def base_rate(self) -> np.ndarray:
        """float64 ``[n, T]``: the observation's exceeding pixels over ALL pixels of the plane (NaN for empty planes)."""
        obs, pix = _host(self.observed).astype(np.float64), _host(self.pixels).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(pix[:, None] > 0, obs / pix[:, None], np.nan)

    def useful(self) -> np.ndarray:
        """float64 ``[n, T]``: ``0.5 + base_rate / 2``, the FSS above which a scale is called useful (Roberts and Lean 2008)."""
        return 0.5 + self.base_rate() / 2.0


class Verification(NamedTuple):
    """What :func:`verify_nowcast` returns: a :class:`ContingencyTable` and :class:`FSSSums`, one row per plane (lead)."""
    contingency: ContingencyTable
    fss: FSSSums

    def __add__(self, other):
        if not isinstance(other, Verification):
            return NotImplemented
        return Verification(self.contingency + other.contingency, self.fss + other.fss)


class VerifierFrame(NamedTuple):
    """What :meth:`NowcastVerifier.update` returns.  ``frame`` the index of this scan; ``verified`` the lead frames whose
    forecasts were verified against it; ``source`` float32 ``[h, w]`` the plane the forecasts of this scan were issued from
    (this scan, NaN under its mask) -- it IS the persistence forecast for every lead; ``forecasts`` float32 ``[L, h, w]`` the
    nowcasts filed for frames ``frame + lead_frames[l]``, ``None`` while there is no motion to issue one; ``motion`` the
    motion they moved along (a filled :class:`MotionGrid`, the given field, or ``None``)."""
    frame: int
    verified: Tuple[int, ...]
    source: object
    forecasts: object
    motion: object


def _host(t) -> np.ndarray:
    return t.detach().cpu().numpy() if _is_tensor(t) else np.asarray(t)


# ---- validation (host only) --------------------------------------------------------------------------------------------------
def _check_thresholds(thresholds) -> np.ndarray:
    """1 .. 8 finite thresholds as the float32 values the kernels compare with."""
    try:
        values = [float(v) for v in (thresholds if hasattr(thresholds, "__iter__") else (thresholds,))]
    except (TypeError, ValueError):
        raise ValueError(f"thresholds must be numbers, got {thresholds!r}") from None
    if not 1 <= len(values) <= MAX_THRESHOLDS:
        raise ValueError(f"thresholds: 1 .. {MAX_THRESHOLDS} per call, got {len(values)}")
    with np.errstate(over="ignore"):
        out = np.asarray(values, dtype=np.float64).astype(np.float32)
    if not np.isfinite(out).all():
        raise ValueError(f"thresholds must be finite float32 values, got {values!r}")
    return out


def _check_scale(scale, what="scale") -> int:
    if not _is_int(scale) or not 1 <= scale <= MAX_SCALE:
        raise ValueError(f"{what} must be an integer in 1 .. {MAX_SCALE}, not {scale!r}")
    return int(scale)


def _check_scales(scales) -> Tuple[int, ...]:
    if not hasattr(scales, "__iter__"):
        scales = (scales,)
    scales = tuple(scales)
    if not 1 <= len(scales) <= MAX_SCALES:
        raise ValueError(f"scales: 1 .. {MAX_SCALES} per call, got {len(scales)}")
    return tuple(_check_scale(n, "scales: every window size") for n in scales)


def _check_pair(forecast, observed, mask, names=("forecast", "observed")):
    shape3 = _check_planes(forecast, names[0])
    if _check_planes(observed, names[1]) != shape3 or tuple(forecast.shape) != tuple(observed.shape):
        raise ValueError(f"{names[0]} of shape {list(forecast.shape)} and {names[1]} of shape {list(observed.shape)} differ")
    _check_mask(mask, forecast, "mask")
    return shape3


def _c_thresholds(thr: np.ndarray):
    return (_native.c_float * len(thr))(*[float(v) for v in thr])


# ---- device ------------------------------------------------------------------------------------------------------------------
def _contingency(lib, torch, f, o, m, shape3, thr) -> ContingencyTable:
    n = shape3[0]
    counts = torch.empty((n, len(thr), 3), dtype=torch.int64, device=f.device)
    valid = torch.empty((n,), dtype=torch.int64, device=f.device)
    _native.check(lib.rg_contingency_f32(_native.ptr(f), _native.ptr(o), _native.ptr(m), *shape3, _c_thresholds(thr), len(thr),
                                         _native.ptr(counts), _native.ptr(valid), _native.stream_ptr()), "rg_contingency_f32")
    hits, fa, miss = counts[..., 0], counts[..., 1], counts[..., 2]
    return ContingencyTable(hits, fa, miss, valid[:, None] - hits - fa - miss, valid)


def _sat(lib, torch, src, partner, m, shape3, thr):
    sat = torch.empty((shape3[0], len(thr), shape3[1], shape3[2]), dtype=torch.int32, device=src.device)
    _native.check(lib.rg_exceedance_sat_i32(_native.ptr(src), _native.ptr(partner), _native.ptr(m), *shape3, _c_thresholds(thr),
                                            len(thr), _native.ptr(sat), _native.stream_ptr()), "rg_exceedance_sat_i32")
    return sat


def _fss(lib, torch, f, o, m, shape3, thr, scales) -> FSSSums:
    n, h, w = shape3
    sat_f, sat_o = _sat(lib, torch, f, o, m, shape3, thr), _sat(lib, torch, o, f, m, shape3, thr)
    sums = torch.empty((n, len(thr), len(scales), 3), dtype=torch.int64, device=f.device)
    _native.check(lib.rg_fss_sums_i32(_native.ptr(sat_f), _native.ptr(sat_o), n * len(thr), h, w,
                                      (_native.c_int32 * len(scales))(*scales), len(scales), _native.ptr(sums),
                                      _native.stream_ptr()), "rg_fss_sums_i32")
    if h and w:
        observed = sat_o[:, :, h - 1, w - 1].to(torch.int64)           # the table's last entry: every exceeding pixel
    else:
        observed = torch.zeros((n, len(thr)), dtype=torch.int64, device=f.device)
    return FSSSums(sums, observed, torch.full((n,), h * w, dtype=torch.int64, device=f.device))


def _check_layers(n, thr):
    if n * len(thr) > 65535:
        raise ValueError(f"planes: {n} planes x {len(thr)} thresholds are more than 65535 layers per call")


def _stage(forecast, observed, mask):
    """The three operands as contiguous device tensors (mask may be None)."""
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(forecast, observed, mask)
    f = _to_device(forecast, dev)
    o = None if observed is None else _to_device(observed, dev)
    m = None if mask is None else _to_device(mask, dev, torch.uint8)
    return torch, lib, dev, f, o, m


def contingency_device(forecast, observed, thresholds, mask=None) -> ContingencyTable:
    """Hits, false alarms, misses and correct negatives of ``forecast`` against ``observed`` at each of ``thresholds``
    (``rg_contingency_f32``).  ``forecast`` / ``observed``: float32 ``[h, w]`` or ``[n, h, w]`` of one shape (``n`` leads or
    scans, each verified on its own); ``thresholds``: 1 .. 8 finite numbers, compared as float32 with ``>=``; ``mask``
    (optional): non-zero leaves the pixel out.  A pixel that is NaN in either field is left out of both.  Returns a
    :class:`ContingencyTable` of int64 device tensors ``[n, T]`` (``n = 1`` for single planes)."""
    shape3 = _check_pair(forecast, observed, mask)
    thr = _check_thresholds(thresholds)
    if shape3[0] > 65535:
        raise ValueError(f"forecast: at most 65535 planes per call, got {shape3[0]}")
    torch, lib, dev, f, o, m = _stage(forecast, observed, mask)
    with torch.cuda.device(dev):
        return _contingency(lib, torch, f, o, m, shape3, thr)


def categorical_scores(table: ContingencyTable) -> dict:
    """The categorical scores of a :class:`ContingencyTable` as float64 arrays ``[n, T]`` on the host (this reads the table
    back).  With ``a`` hits, ``b`` false alarms, ``c`` misses, ``d`` correct negatives and ``N = a + b + c + d``:

    ``pod = a / (a + c)``; ``far = b / (a + b)``; ``csi = a / (a + b + c)``; ``bias = (a + b) / (a + c)``;
    ``ets = (a - r) / (a + b + c - r)`` with ``r = (a + b)(a + c) / N``;
    ``hss = 2 (a d - b c) / ((a + c)(c + d) + (a + b)(b + d))``; ``base_rate = (a + c) / N``.

    A zero denominator gives NaN, never an exception."""
    if not isinstance(table, ContingencyTable):
        raise ValueError(f"table must be a ContingencyTable, not {type(table).__name__}")
    a, b, c, d = (_host(t).astype(np.float64) for t in (table.hits, table.false_alarms, table.misses, table.correct_negatives))
    n = a + b + c + d

    def ratio(num, den):
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(den != 0, num / np.where(den != 0, den, 1.0), np.nan)

    r = ratio((a + b) * (a + c), n)
    return dict(pod=ratio(a, a + c), far=ratio(b, a + b), csi=ratio(a, a + b + c), bias=ratio(a + b, a + c),
                ets=ratio(a - r, a + b + c - r), hss=ratio(2.0 * (a * d - b * c), (a + c) * (c + d) + (a + b) * (b + d)),
                base_rate=ratio(a + c, n))


def exceedance_sat_device(planes, thresholds, partner=None, mask=None):
    """The inclusive summed-area tables of the threshold exceedances of ``planes`` (``rg_exceedance_sat_i32``): int32
    ``[n, T, h, w]`` with ``sat[p, t, y, x]`` = the exceeding pixels of plane ``p`` at ``y' <= y, x' <= x``.  ``partner``
    (optional, float32 of the planes' shape) supplies only validity -- a pixel whose partner is NaN exceeds nothing, which is
    how a forecast and an observation mask each other; ``mask`` as in :func:`contingency_device`."""
    shape3 = _check_planes(planes, "planes")
    if partner is not None and (_check_planes(partner, "partner") != shape3 or tuple(partner.shape) != tuple(planes.shape)):
        raise ValueError(f"partner of shape {list(partner.shape)} for planes of shape {list(planes.shape)}")
    _check_mask(mask, planes, "mask")
    thr = _check_thresholds(thresholds)
    _check_layers(shape3[0], thr)
    torch, lib, dev, src, other, m = _stage(planes, partner, mask)
    with torch.cuda.device(dev):
        return _sat(lib, torch, src, other, m, shape3, thr)


def neighbourhood_fraction_device(planes, thresholds, scale: int, mask=None):
    """The fraction of the ``scale`` x ``scale`` neighbourhood of every pixel that is at or above each threshold: float32
    ``[n, T, h, w]``, ``count / scale^2`` with the plane zero-padded beyond its rim (``rg_exceedance_sat_i32``, then
    ``rg_box_fraction_f32``) -- "the probability of at least 35 dBZ within ``scale`` pixels" of a deterministic nowcast.  NaN
    and masked pixels count as no exceedance.  At ``scale=1`` it is the 0/1 exceedance itself."""
    shape3 = _check_planes(planes, "planes")
    _check_mask(mask, planes, "mask")
    thr = _check_thresholds(thresholds)
    scale = _check_scale(scale)
    _check_layers(shape3[0], thr)
    torch, lib, dev, src, _, m = _stage(planes, None, mask)
    n, h, w = shape3
    with torch.cuda.device(dev):
        sat = _sat(lib, torch, src, None, m, shape3, thr)
        out = torch.empty((n, len(thr), h, w), dtype=torch.float32, device=dev)
        _native.check(lib.rg_box_fraction_f32(_native.ptr(sat), n * len(thr), h, w, scale, _native.ptr(out), _native.stream_ptr()),
                      "rg_box_fraction_f32")
    return out


def fss_device(forecast, observed, thresholds, scales, mask=None) -> FSSSums:
    """The sums of the fractions skill score of ``forecast`` against ``observed`` for every threshold and every window size
    of ``scales`` (1 .. 16 integers in 1 .. 255): two :func:`exceedance_sat_device` tables, each field the other's partner,
    then ``rg_fss_sums_i32``.  Returns :class:`FSSSums`; ``.fss()`` is the score, ``.useful()`` the level it has to reach."""
    shape3 = _check_pair(forecast, observed, mask)
    thr = _check_thresholds(thresholds)
    scales = _check_scales(scales)
    _check_layers(shape3[0], thr)
    torch, lib, dev, f, o, m = _stage(forecast, observed, mask)
    with torch.cuda.device(dev):
        return _fss(lib, torch, f, o, m, shape3, thr, scales)


def verify_nowcast(forecasts, observations, thresholds, scales, mask=None) -> Verification:
    """Contingency counts and FSS sums of ``forecasts`` against ``observations`` -- float32 ``[L, h, w]`` (or ``[h, w]``), one
    pair per lead -- in one call: a :class:`Verification` whose members hold one row per lead.  ``mask`` (optional) has the
    planes' shape.  Nothing synchronises with the host until the caller reads a result."""
    shape3 = _check_pair(forecasts, observations, mask, ("forecasts", "observations"))
    thr = _check_thresholds(thresholds)
    scales = _check_scales(scales)
    _check_layers(shape3[0], thr)
    torch, lib, dev, f, o, m = _stage(forecasts, observations, mask)
    with torch.cuda.device(dev):
        return Verification(_contingency(lib, torch, f, o, m, shape3, thr), _fss(lib, torch, f, o, m, shape3, thr, scales))


class NowcastVerifier:
    """Verification along a sequence of scans: feed it one plane per scan; every forecast it issued for this scan is verified
    against it, the advection nowcast and the persistence forecast alike, and the integer sums are added to per-lead totals
    on the device.

    ``lead_frames``: the leads in whole scans (1 .. 16 distinct positive integers).  ``thresholds`` / ``scales``: as for
    :func:`verify_nowcast`.  ``motion``: ``"auto"`` estimates the motion between the previous and the current plane
    (:func:`estimate_motion_device`, then :func:`fill_motion_device` with ``min_score``; ``block``, ``stride``, ``search``,
    ``lo``, ``hi``, ``min_echo`` go to the estimate) -- the first scan then issues nothing; ``None`` is zero motion (the
    nowcast IS persistence); a filled :class:`MotionGrid` or a ``(field, lattice)`` pair is used as it is for every scan.
    ``method`` and ``substeps`` go to :func:`advect_device`.  Forecast pixels that come from outside the plane are NaN, and so
    are pixels under the issuing scan's mask: they are left out of BOTH fields when the forecast is verified, as are the pixels
    under the verifying scan's mask.

    Nothing here synchronises with the host except :meth:`scores`."""

    def __init__(self, lead_frames, thresholds, scales, motion="auto", *, min_score: float = 0.5, **nowcast_kw):
        try:
            leads = tuple(lead_frames) if hasattr(lead_frames, "__iter__") else (lead_frames,)
        except TypeError:
            leads = ()
        if not 1 <= len(leads) <= MAX_LEADS or not all(_is_int(v) and v >= 1 for v in leads) or len(set(leads)) != len(leads):
            raise ValueError(f"lead_frames must be 1 .. {MAX_LEADS} distinct positive integers, got {lead_frames!r}")
        self.lead_frames = tuple(int(v) for v in leads)
        self.thresholds = _check_thresholds(thresholds)
        self.scales = _check_scales(scales)
        unknown = sorted(set(nowcast_kw) - set(_VERIFIER_ESTIMATE_KEYS) - set(_VERIFIER_ADVECT_KEYS))
        if unknown:
            raise ValueError(f"unknown keyword(s) {unknown}: expected some of "
                             f"{list(_VERIFIER_ESTIMATE_KEYS + _VERIFIER_ADVECT_KEYS)}")
        self._advect = {k: v for k, v in nowcast_kw.items() if k in _VERIFIER_ADVECT_KEYS}
        estimate = {k: v for k, v in nowcast_kw.items() if k in _VERIFIER_ESTIMATE_KEYS}
        if self._advect.get("method", "nearest") not in ADVECT_METHODS:
            raise ValueError(f"method must be one of {sorted(ADVECT_METHODS)}, not {self._advect['method']!r}")
        substeps = self._advect.get("substeps", 1)
        if not _is_int(substeps) or not 1 <= substeps <= MAX_SUBSTEPS:
            raise ValueError(f"substeps must be an integer in 1 .. {MAX_SUBSTEPS}, not {substeps!r}")
        self._lattice = None
        if isinstance(motion, str):
            if motion != "auto":
                raise ValueError(f"motion must be 'auto', None, a MotionGrid or (field, lattice), not {motion!r}")
            _check_blocks(estimate.get("block", 32), estimate.get("stride", 16), estimate.get("search", 16), estimate.get("min_echo"))
            _check_levels(estimate.get("lo", 0.0), estimate.get("hi", 63.5))
        else:
            if estimate:
                raise ValueError(f"{sorted(estimate)} belong to the motion estimate, which motion={type(motion).__name__} does not run")
            if isinstance(motion, tuple) and not isinstance(motion, MotionGrid):
                if len(motion) != 2:
                    raise ValueError("a given motion is a MotionGrid or the pair (field, lattice)")
                motion, self._lattice = motion
            if motion is not None and not isinstance(motion, MotionGrid) and not hasattr(motion, "shape"):
                raise ValueError(f"motion must be 'auto', None, a MotionGrid or (field, lattice), not {type(motion).__name__}")
        self.motion = motion
        self._estimate = estimate
        self.min_score = float(min_score)
        if math.isnan(self.min_score):
            raise ValueError("min_score must not be NaN")
        self.reset()

    def reset(self) -> None:
        """Forget every scan, pending forecast and total."""
        self._frame = 0
        self._last = None                    # (plane tensor, mask tensor or None) of the previous scan
        self._pending = {}                   # target frame -> [(lead index, nowcast plane or None, persistence plane)]
        self._totals = {"nowcast": None, "persistence": None}       # Verification with one row per lead
        self._counts = {"nowcast": [0] * len(self.lead_frames), "persistence": [0] * len(self.lead_frames)}

    def _add(self, kind, rows, result: Verification) -> None:
        """Add row ``j`` of ``result`` to the totals of lead ``rows[j]``."""
        torch = _native.torch_mod()
        L = len(self.lead_frames)
        for j, row in enumerate(rows):
            self._counts[kind][row] += 1
        if rows != list(range(L)):                                   # spread over the leads; the others add zero
            def spread(t):
                full = torch.zeros((L,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
                for j, row in enumerate(rows):
                    full[row] = t[j]
                return full
            result = Verification(ContingencyTable(*(spread(t) for t in result.contingency)),
                                  FSSSums(*(spread(t) for t in result.fss)))
        total = self._totals[kind]
        self._totals[kind] = result if total is None else total + result

    def update(self, plane, mask=None) -> VerifierFrame:
        """Take the next scan: ``plane`` float32 ``[h, w]``, ``mask`` (optional) non-zero where the radar does not see.
        Verifies what is pending for this scan, then issues and files the forecasts from it.  Returns a
        :class:`VerifierFrame`."""
        if _check_planes(plane, "plane")[0] != 1 or len(plane.shape) != 2:
            raise ValueError("plane must be one float32 [h, w] plane")
        _check_mask(mask, plane, "mask")
        shape = tuple(int(v) for v in plane.shape)
        if self._last is not None and tuple(self._last[0].shape) != shape:
            raise ValueError(f"plane of shape {list(shape)} after planes of {list(self._last[0].shape)}")
        if not isinstance(self.motion, str) and self.motion is not None:
            _check_field(self.motion, self._lattice, shape)
        torch = _native.torch_mod()
        dev = _device_of(plane, mask) if self._last is None else self._last[0].device
        obs = _to_device(plane, dev)
        mask_t = None if mask is None else _to_device(mask, dev, torch.uint8)
        k = self._frame
        # 1. verify what was filed for this scan
        due = sorted(self._pending.pop(k, []), key=lambda e: e[0])
        for kind, column in (("nowcast", 1), ("persistence", 2)):
            held = [e for e in due if e[column] is not None]
            if not held:
                continue
            stack = torch.stack([e[column] for e in held])
            target = obs.unsqueeze(0).expand(len(held), -1, -1)
            masks = None if mask_t is None else mask_t.unsqueeze(0).expand(len(held), -1, -1)
            self._add(kind, [e[0] for e in held], verify_nowcast(stack, target, self.thresholds, self.scales, masks))
        # 2. issue the forecasts of this scan
        source = obs if mask_t is None else torch.where(mask_t != 0, torch.full((), float("nan"), device=dev), obs)
        last, self._last = self._last, (obs, mask_t)
        forecasts, motion = None, None
        if isinstance(self.motion, str):
            if last is not None:
                grid = estimate_motion_device(last[0], obs, mask_prev=last[1], mask_next=mask_t, **self._estimate)
                motion = fill_motion_device(grid, self.min_score)
                forecasts = advect_device(source, motion, self.lead_frames, fill_value=float("nan"), **self._advect)
        elif self.motion is None:
            forecasts = source.unsqueeze(0).expand(len(self.lead_frames), -1, -1).contiguous()
        else:
            motion = self.motion
            forecasts = advect_device(source, motion, self.lead_frames, lattice=self._lattice, fill_value=float("nan"), **self._advect)
        for li, lead in enumerate(self.lead_frames):
            self._pending.setdefault(k + lead, []).append((li, None if forecasts is None else forecasts[li], source))
        self._frame = k + 1
        return VerifierFrame(k, tuple(self.lead_frames[e[0]] for e in due), source, forecasts, motion)

    def totals(self, kind: str = "nowcast") -> Optional[Verification]:
        """The :class:`Verification` totals of ``"nowcast"`` or ``"persistence"``, one row per lead on the device; ``None``
        before anything was verified."""
        if kind not in self._totals:
            raise ValueError(f"kind must be 'nowcast' or 'persistence', not {kind!r}")
        return self._totals[kind]

    def scores(self) -> dict:
        """Scores per lead for the nowcast and for persistence (reads the totals back): ``{"lead_frames", "thresholds",
        "scales", "nowcast": {...}, "persistence": {...}}``, each inner dict holding ``verified`` (forecasts per lead), the
        arrays of :func:`categorical_scores` ``[L, T]``, ``fss [L, T, S]`` and ``useful [L, T]``; ``None`` for a kind of which
        nothing was verified yet."""
        out = dict(lead_frames=self.lead_frames, thresholds=tuple(float(t) for t in self.thresholds), scales=self.scales)
        for kind, total in self._totals.items():
            if total is None:
                out[kind] = None
                continue
            out[kind] = dict(categorical_scores(total.contingency), fss=total.fss.fss(), useful=total.fss.useful(),
                             verified=tuple(self._counts[kind]))
        return out
