"""Probabilistic nowcasts on the device (include/radargrid_ensemble.h; kernels in csrc/rg_ensemble.hip): the probability of
reaching a threshold at a lead time, from an ensemble of extrapolations whose motion is perturbed with an error that grows
with the lead, and the scores such a forecast is judged by.

* :func:`motion_perturbations` draws the members' displacement errors per lead (host);
* :func:`ensemble_exceedance_device` samples, thresholds and counts all members in ONE kernel
  (``rg_ensemble_exceedance_f32``) and returns :class:`EnsembleProducts` -- the ``M x L`` member planes are never stored;
* :func:`probabilistic_nowcast_device` chains the motion estimate, the fill, the perturbations along the mean motion and the
  ensemble; :func:`probabilistic_nowcast` is its NumPy-in, NumPy-out wrapper;
* :func:`ensemble_histogram_device` counts, per lead and threshold, how often ``k`` of ``M`` members exceeded and how often the
  observation then did (``rg_ensemble_histogram_u8``): a :class:`ProbabilityTable` of integers that adds over scans;
* :func:`probability_scores` turns the table into the Brier score with its reliability, resolution and uncertainty terms, the
  Brier skill score, the reliability curve, the sharpness counts and the ROC (host float64, from the integers alone).

SIGN AND UNITS are those of :mod:`.motion`: echo at pixel ``p`` is found at ``p + motion`` one interval later, vectors are
``(dy, dx)`` in pixels per interval, leads are in intervals.  Member ``m`` at lead ``l`` samples the plane at
``p - d - shifts[l, m]``, with ``d`` the displacement :func:`~radar_processor_amd.motion.advect_device` uses -- with all
shifts zero every member IS that nowcast, bit for bit.

The device functions take tensors or ndarrays, enqueue on torch's current stream and validate every argument before the
device is touched.  Only :func:`probabilistic_nowcast_device` reads back from the device (the mean motion vector, two numbers,
which the host-side perturbations need).  The kernels are pinned to the NumPy restatement of the header's formulas
(``tests/ensemble_oracle.py``): integers equal, ``prob`` and ``mean`` bit for bit.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Tuple

import numpy as np

from . import _native
from .motion import (_ESTIMATE_KEYS, ADVECT_METHODS, MAX_SUBSTEPS, _check_field, _check_leads, _check_mask,
                     _check_planes, _device_of, _dtype_name, _is_int, _is_tensor, _to_device, estimate_motion_device,
                     fill_motion_device)
from .verification import _c_thresholds, _check_thresholds, _host

MAX_MEMBERS = _native.RG_MAX_MEMBERS
WANT = ("prob", "counts", "members", "mean")
_ENSEMBLE_KEYS = ("method", "substeps", "min_members", "want")


class EnsembleProducts(NamedTuple):
    """What :func:`ensemble_exceedance_device` returns; a product that was not asked for is ``None``.  ``prob`` float32
    ``[L, T, h, w]``: the fraction of the present members at or above threshold ``t``, NaN where fewer than ``min_members``
    are present; ``counts`` uint8 ``[L, T, h, w]``: how many are; ``members`` uint8 ``[L, h, w]``: how many are present;
    ``mean`` float32 ``[L, h, w]``: their mean, NaN below ``min_members``.  ``thresholds`` float32 ndarray ``[T]``, ``leads`` a
    tuple of floats, ``n_members`` the ensemble size ``M``."""
    prob: object
    counts: object
    members: object
    mean: object
    thresholds: np.ndarray
    leads: Tuple[float, ...]
    n_members: int


class ProbabilityTable(NamedTuple):
    """What :func:`ensemble_histogram_device` returns, int64 on the device.  ``hist [n, T, M + 1, 2]``: ``hist[p, t, k, o]`` is
    the number of valid pixels of plane (lead) ``p`` where ``k`` of the ``M`` members reached threshold ``t`` and the observation
    did (``o = 1``) or did not (``o = 0``); ``valid [n]`` the valid pixels.  ``a + b`` adds two tables of one shape, ensemble size
    and thresholds exactly (more scans of the same leads)."""
    hist: object
    valid: object
    n_members: int
    thresholds: np.ndarray

    def __add__(self, other):
        if not isinstance(other, ProbabilityTable):
            return NotImplemented
        if tuple(self.hist.shape) != tuple(other.hist.shape) or self.n_members != other.n_members:
            raise ValueError(f"tables of {list(self.hist.shape)} and {list(other.hist.shape)} (planes, thresholds, M + 1, 2) do not add")
        if not np.array_equal(np.asarray(self.thresholds), np.asarray(other.thresholds)):
            raise ValueError(f"tables at thresholds {list(self.thresholds)} and {list(other.thresholds)} do not add")
        return ProbabilityTable(self.hist + other.hist, self.valid + other.valid, self.n_members, self.thresholds)


# ---- validation (host only) --------------------------------------------------------------------------------------------------
def _check_members(n_members) -> int:
    if not _is_int(n_members) or not 1 <= n_members <= MAX_MEMBERS:
        raise ValueError(f"n_members must be an integer in 1 .. {MAX_MEMBERS}, not {n_members!r}")
    return int(n_members)


def _check_growth(triple, what: str) -> Tuple[float, float, float]:
    """``(a, b, c)`` of the speed error ``a * t**b + c``: finite, ``b > -1`` so that its integral from 0 exists."""
    try:
        a, b, c = (float(v) for v in triple)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be three numbers (a, b, c) of the speed error a * t**b + c, got {triple!r}") from None
    if not all(math.isfinite(v) for v in (a, b, c)) or b <= -1.0:
        raise ValueError(f"{what}: a, b and c must be finite with b > -1, got {(a, b, c)!r}")
    return a, b, c


def _check_shifts(shifts, n_leads: int) -> int:
    """float64 ``[L, M, 2]`` for ``L`` leads; returns ``M``.  An ndarray must be finite; for a tensor that is the caller's duty."""
    if not hasattr(shifts, "shape") or not hasattr(shifts, "dtype") or _dtype_name(shifts) != "float64" or len(shifts.shape) != 3 \
            or int(shifts.shape[2]) != 2:
        raise ValueError("shifts must be float64 [n_leads, n_members, 2] = (sy, sx) in pixels (motion_perturbations)")
    if int(shifts.shape[0]) != n_leads:
        raise ValueError(f"shifts of shape {list(shifts.shape)} for {n_leads} leads")
    n_members = int(shifts.shape[1])
    if not 1 <= n_members <= MAX_MEMBERS:
        raise ValueError(f"shifts: 1 .. {MAX_MEMBERS} members per call, got {n_members}")
    if not _is_tensor(shifts) and not np.isfinite(shifts).all():
        raise ValueError("shifts hold NaN or inf")
    return n_members


def _check_ensemble(method, substeps, min_members, want, n_members) -> Tuple[str, ...]:
    if method not in ADVECT_METHODS:
        raise ValueError(f"method must be one of {sorted(ADVECT_METHODS)}, not {method!r}")
    if not _is_int(substeps) or not 1 <= substeps <= MAX_SUBSTEPS:
        raise ValueError(f"substeps must be an integer in 1 .. {MAX_SUBSTEPS}, not {substeps!r}")
    if not _is_int(min_members) or not 1 <= min_members <= n_members:
        raise ValueError(f"min_members must be an integer in 1 .. n_members = {n_members}, not {min_members!r}")
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(name not in WANT for name in want) or len(set(want)) != len(want):
        raise ValueError(f"want must name some of {list(WANT)}, each once; got {list(want)}")
    return want


def _check_plane(plane, what: str) -> Tuple[int, int]:
    if _check_planes(plane, what)[0] != 1 or len(plane.shape) != 2:
        raise ValueError(f"{what} must be one float32 [h, w] plane")
    return int(plane.shape[0]), int(plane.shape[1])


# ---- host: the perturbations ---------------------------------------------------------------------------------------------------
def motion_perturbations(n_members: int, leads, *, direction, par, perp, seed, control: bool = True) -> np.ndarray:
    """The members' displacement errors: float64 ``[L, M, 2]`` = ``(sy, sx)`` in pixels for ``leads`` (in intervals), the
    ``shifts`` of :func:`ensemble_exceedance_device`.

    The error of the motion is modelled as a speed error that grows with the lead, ``s(t) = a * t**b + c`` in pixels per
    interval with ``t`` in intervals, given separately along ``direction`` (``par = (a, b, c)``) and perpendicular to it
    (``perp``); both are REQUIRED -- they are fitted to a radar network's own motion errors, and there is no default that fits
    all ("Probabilistic nowcasts", converts published km/h-and-minutes figures).  Per member two standard
    normal numbers ``(z_par, z_perp)`` are drawn ONCE from ``np.random.default_rng(seed)`` -- a member errs in the same sense
    at every lead -- and are ``(0, 0)`` for member 0 when ``control`` (the unperturbed nowcast).  The displacement error at lead
    ``L`` is the speed error integrated from 0:

        ``z * (a * L**(b + 1) / (b + 1) + c * L)``        (odd in ``L``: a negative lead mirrors the positive one)

    along the unit vector of ``direction`` -- a ``(dy, dx)`` vector, normally the mean of the filled motion field -- and along
    its perpendicular ``(dx, -dy)``.  A zero ``direction`` counts as ``(0, 1)``, eastward.

    This is the FORM of pysteps' "bps" motion perturbation (Bowler, Pierce and Seed 2006); parity with pysteps is unpinned: the
    random stream, the order of the draws and the units are this function's own."""
    n_members = _check_members(n_members)
    leads = np.asarray(_check_leads(leads), dtype=np.float64)
    par, perp = _check_growth(par, "par"), _check_growth(perp, "perp")
    try:
        dy, dx = (float(v) for v in direction)
    except (TypeError, ValueError):
        raise ValueError(f"direction must be a (dy, dx) vector, got {direction!r}") from None
    if not (math.isfinite(dy) and math.isfinite(dx)):
        raise ValueError(f"direction must be finite, got {direction!r}")
    norm = math.hypot(dy, dx)
    e_par = np.array([dy / norm, dx / norm]) if norm > 0.0 else np.array([0.0, 1.0])
    e_perp = np.array([e_par[1], -e_par[0]])
    z = np.random.default_rng(seed).standard_normal((n_members, 2))
    if control:
        z[0] = 0.0

    def grown(abc):
        a, b, c = abc
        t = np.abs(leads)
        return np.sign(leads) * (a * t ** (b + 1.0) / (b + 1.0) + c * t)

    amp_par, amp_perp = grown(par), grown(perp)                                           # [L]
    return (z[None, :, 0, None] * amp_par[:, None, None] * e_par[None, None, :]
            + z[None, :, 1, None] * amp_perp[:, None, None] * e_perp[None, None, :])


# ---- device ------------------------------------------------------------------------------------------------------------------
def ensemble_exceedance_device(plane, motion, leads, shifts, thresholds, *, lattice=None, method: str = "nearest",
                               substeps: int = 1, min_members: int = 1, want=("prob",)) -> EnsembleProducts:
    """The exceedance probabilities of an ensemble of extrapolations of ``plane`` (``rg_ensemble_exceedance_f32``).

    ``plane``: float32 ``[h, w]``; ``motion``, ``lattice``, ``leads`` (at most 16), ``method`` and ``substeps`` as in
    :func:`~radar_processor_amd.motion.advect_device`; ``shifts``: float64 ``[L, M, 2]`` = ``(sy, sx)`` in pixels, member
    ``m``'s extra displacement at lead ``l`` (:func:`motion_perturbations`; ``M`` in 1 .. 64; finite -- checked for an
    ndarray, the caller's duty for a tensor, where a NaN shift makes that member missing everywhere); ``thresholds``: 1 .. 8
    finite numbers, compared as float32 with ``>=``.

    Member ``m`` at lead ``l`` is ``plane`` sampled at ``p - d - shifts[l, m]``; it is MISSING at a pixel where that sample is
    NaN (outside the plane, or the plane's own NaN).  ``want`` names the products to compute, some of ``"prob"``,
    ``"counts"``, ``"members"``, ``"mean"`` (see :class:`EnsembleProducts`); ``prob`` and ``mean`` are NaN where fewer than
    ``min_members`` members are present.  One kernel forms everything; no member plane is stored."""
    h, w = _check_plane(plane, "plane")
    field, lat = _check_field(motion, lattice, (h, w))
    leads = _check_leads(leads)
    n_members = _check_shifts(shifts, len(leads))
    thr = _check_thresholds(thresholds)
    want = _check_ensemble(method, substeps, min_members, want, n_members)
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(plane, field, shifts)
    src, field, sh = _to_device(plane, dev), _to_device(field, dev), _to_device(shifts, dev)
    L, T = len(leads), len(thr)
    shapes = dict(prob=((L, T, h, w), torch.float32), counts=((L, T, h, w), torch.uint8), members=((L, h, w), torch.uint8),
                  mean=((L, h, w), torch.float32))
    out = {name: torch.empty(shapes[name][0], dtype=shapes[name][1], device=dev) if name in want else None for name in WANT}
    if leads:                                                                # an empty tensor has no address to pass
        with torch.cuda.device(dev):
            _native.check(lib.rg_ensemble_exceedance_f32(
                _native.ptr(src), h, w, _native.ptr(field), _native.MotionLattice(*lat), (_native.c_double * L)(*leads), L,
                int(substeps), ADVECT_METHODS[method], _native.ptr(sh), n_members, _c_thresholds(thr), T, int(min_members),
                _native.ptr(out["prob"]), _native.ptr(out["counts"]), _native.ptr(out["members"]), _native.ptr(out["mean"]),
                _native.stream_ptr()), "rg_ensemble_exceedance_f32")
    return EnsembleProducts(out["prob"], out["counts"], out["members"], out["mean"], thr, leads, n_members)


def probabilistic_nowcast_device(prev, next, leads, thresholds, n_members: int, *, par, perp, seed, control: bool = True,
                                 min_score: float = 0.5, **kw):
    """The probabilities of ``next`` reaching ``thresholds`` after ``leads`` intervals, from ``n_members`` extrapolations along
    the motion between ``prev`` and ``next`` (two float32 planes ``[h, w]``):
    :func:`~radar_processor_amd.motion.estimate_motion_device`, :func:`~radar_processor_amd.motion.fill_motion_device` with
    ``min_score``, :func:`motion_perturbations` along the mean vector of the filled field (``par``, ``perp``, ``seed``,
    ``control``), then :func:`ensemble_exceedance_device` of ``next``.  Keywords go to the stage that names them (``block``,
    ``stride``, ``search``, ``lo``, ``hi``, ``min_echo``, ``mask_prev``, ``mask_next``; ``method``, ``substeps``,
    ``min_members``, ``want``).  Returns ``(EnsembleProducts, the filled MotionGrid)`` on the device.  Reading the mean vector
    back waits for the motion estimate: the one host synchronisation of this module."""
    unknown = sorted(set(kw) - set(_ESTIMATE_KEYS) - set(_ENSEMBLE_KEYS))
    if unknown:
        raise ValueError(f"unknown keyword(s) {unknown}: expected some of {list(_ESTIMATE_KEYS + _ENSEMBLE_KEYS)}")
    for name, a in (("prev", prev), ("next", next)):
        _check_plane(a, name)
    leads = _check_leads(leads)
    n_members = _check_members(n_members)
    thr = _check_thresholds(thresholds)
    _check_growth(par, "par"), _check_growth(perp, "perp")
    if math.isnan(float(min_score)):
        raise ValueError("min_score must not be NaN")
    ens_kw = {k: v for k, v in kw.items() if k in _ENSEMBLE_KEYS}
    _check_ensemble(ens_kw.get("method", "nearest"), ens_kw.get("substeps", 1), ens_kw.get("min_members", 1),
                    ens_kw.get("want", ("prob",)), n_members)
    grid = estimate_motion_device(prev, next, **{k: v for k, v in kw.items() if k in _ESTIMATE_KEYS})
    grid = fill_motion_device(grid, min_score)
    direction = grid.motion.to(_native.torch_mod().float64).mean(dim=(0, 1)).cpu().numpy()
    shifts = motion_perturbations(n_members, leads, direction=direction, par=par, perp=perp, seed=seed, control=control)
    return ensemble_exceedance_device(next, grid, leads, shifts, thr, **ens_kw), grid


def probabilistic_nowcast(prev, next, leads, thresholds, n_members: int, **kw):
    """:func:`probabilistic_nowcast_device` for NumPy arrays: ``(EnsembleProducts of ndarrays, MotionGrid of ndarrays)``."""
    products, grid = probabilistic_nowcast_device(prev, next, leads, thresholds, n_members, **kw)
    fields = {name: None if getattr(products, name) is None else getattr(products, name).cpu().numpy() for name in WANT}
    return products._replace(**fields), grid._replace(motion=grid.motion.cpu().numpy(), score=grid.score.cpu().numpy(),
                                                      disp=grid.disp.cpu().numpy())


def ensemble_histogram_device(products: EnsembleProducts, observed, mask=None) -> ProbabilityTable:
    """How often ``k`` of the ``M`` members reached each threshold, and how often ``observed`` then did
    (``rg_ensemble_histogram_u8``).  ``products``: :class:`EnsembleProducts` with ``counts`` and ``members``
    (``want=("prob", "counts", "members")``); ``observed``: float32 ``[L, h, w]``, the plane each lead was made for (``[h, w]``
    for one lead); ``mask`` (optional): non-zero leaves the pixel out.  A pixel counts where the observation is not NaN, the
    mask is 0 and ALL ``M`` members are present -- a forecast from fewer members has other possible values, and would blur the
    bins.  Returns a :class:`ProbabilityTable` of int64 device tensors, one row per lead."""
    if not isinstance(products, EnsembleProducts):
        raise ValueError(f"products must be EnsembleProducts, not {type(products).__name__}")
    if products.counts is None or products.members is None:
        raise ValueError('products hold no counts or no members: ask for want=("prob", "counts", "members")')
    n_members = _check_members(products.n_members)
    thr = _check_thresholds(products.thresholds)
    L, h, w = (int(v) for v in products.members.shape)
    if tuple(int(v) for v in products.counts.shape) != (L, len(thr), h, w) or _dtype_name(products.counts) != "uint8" \
            or _dtype_name(products.members) != "uint8":
        raise ValueError(f"products: counts must be uint8 {[L, len(thr), h, w]} for members uint8 {[L, h, w]}")
    shape3 = _check_planes(observed, "observed")
    if shape3 != (L, h, w):
        raise ValueError(f"observed of shape {list(observed.shape)} for forecasts of {[L, h, w]} (leads, h, w)")
    _check_mask(mask, observed, "mask")
    if L < 1 or L > 65535:
        raise ValueError(f"products: 1 .. 65535 planes per call, got {L}")
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(products.counts, observed, mask)
    counts, members = _to_device(products.counts, dev), _to_device(products.members, dev)
    obs = _to_device(observed, dev)
    m = None if mask is None else _to_device(mask, dev, torch.uint8)
    hist = torch.empty((L, len(thr), n_members + 1, 2), dtype=torch.int64, device=dev)
    valid = torch.empty((L,), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _native.check(lib.rg_ensemble_histogram_u8(_native.ptr(counts), _native.ptr(members), _native.ptr(obs), _native.ptr(m), L, h, w,
                                                   n_members, _c_thresholds(thr), len(thr), _native.ptr(hist), _native.ptr(valid),
                                                   _native.stream_ptr()), "rg_ensemble_histogram_u8")
    return ProbabilityTable(hist, valid, n_members, thr)


# ---- host: the scores ----------------------------------------------------------------------------------------------------------
def probability_scores(table: ProbabilityTable) -> dict:
    """The scores of a :class:`ProbabilityTable` as float64 arrays on the host (this reads the table back), from the integers
    alone.  With ``n_k`` the valid pixels whose forecast was ``p_k = k / M``, ``o_k`` those of them where the event was
    observed, ``N = sum n_k`` and ``obar = sum o_k / N`` (the sample base rate), per plane and threshold ``[n, T]``:

    ``brier = sum_k (o_k (p_k - 1)^2 + (n_k - o_k) p_k^2) / N`` -- the mean of ``(p - o)^2`` over the pixels;
    ``reliability = sum_k n_k (p_k - o_k / n_k)^2 / N``; ``resolution = sum_k n_k (o_k / n_k - obar)^2 / N``;
    ``uncertainty = obar (1 - obar)``; ``brier = reliability - resolution + uncertainty`` EXACTLY (Murphy 1973), because a
    forecast takes only the ``M + 1`` values ``p_k``: there is no within-bin term;
    ``bss = 1 - brier / uncertainty``, the skill against always forecasting ``obar``; ``base_rate = obar``.

    ``forecast_probability [M + 1]`` = ``p_k``; ``reliability_curve [n, T, M + 1]`` = ``o_k / n_k``, the observed frequency
    given the forecast (NaN for an unused ``k``); ``sharpness [n, T, M + 1]`` = ``n_k`` (int64).

    ROC: warning when at least ``j`` members exceed, ``j = 0 .. M + 1``: ``pod [n, T, M + 2]`` = ``sum_{k >= j} o_k / sum o_k``,
    ``pofd`` = ``sum_{k >= j} (n_k - o_k) / sum (n_k - o_k)`` -- from ``(1, 1)`` at ``j = 0`` to ``(0, 0)`` at ``j = M + 1``;
    ``roc_area [n, T]`` the area under them by trapezoids.

    An empty denominator gives NaN, never an exception."""
    if not isinstance(table, ProbabilityTable):
        raise ValueError(f"table must be a ProbabilityTable, not {type(table).__name__}")
    hist = _host(table.hist).astype(np.int64)
    M = int(table.n_members)
    if hist.ndim != 4 or hist.shape[2:] != (M + 1, 2):
        raise ValueError(f"table.hist of shape {list(hist.shape)} for {M} members: expected [n, T, {M + 1}, 2]")
    o_int, n_int = hist[..., 1], hist[..., 0] + hist[..., 1]
    o_k, n_k = o_int.astype(np.float64), n_int.astype(np.float64)
    p_k = np.arange(M + 1, dtype=np.float64) / float(M)

    def ratio(num, den):
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(den != 0, num / np.where(den != 0, den, 1.0), np.nan)

    N, O = n_k.sum(axis=-1), o_k.sum(axis=-1)
    obar = ratio(O, N)
    brier = ratio((o_k * (p_k - 1.0) ** 2 + (n_k - o_k) * p_k ** 2).sum(axis=-1), N)
    freq = ratio(o_k, n_k)                                                   # NaN where k was never forecast
    used = n_k > 0
    rel = ratio(np.where(used, n_k * (p_k - np.where(used, freq, 0.0)) ** 2, 0.0).sum(axis=-1), N)
    with np.errstate(invalid="ignore"):
        res = ratio(np.where(used, n_k * (np.where(used, freq, 0.0) - obar[..., None]) ** 2, 0.0).sum(axis=-1), N)
    unc = obar * (1.0 - obar)
    # at least j members: the sums over k >= j, j = 0 .. M + 1 (the last one empty)
    zeros = np.zeros(hist.shape[:2] + (1,), dtype=np.int64)
    hits = np.concatenate([np.cumsum(o_int[..., ::-1], axis=-1)[..., ::-1], zeros], axis=-1).astype(np.float64)
    false = np.concatenate([np.cumsum((n_int - o_int)[..., ::-1], axis=-1)[..., ::-1], zeros], axis=-1).astype(np.float64)
    pod, pofd = ratio(hits, O[..., None]), ratio(false, (N - O)[..., None])
    area = (0.5 * (pod[..., :-1] + pod[..., 1:]) * (pofd[..., :-1] - pofd[..., 1:])).sum(axis=-1)
    return dict(brier=brier, reliability=rel, resolution=res, uncertainty=unc, bss=1.0 - ratio(brier, unc), base_rate=obar,
                forecast_probability=p_k, reliability_curve=freq, sharpness=n_int, pod=pod, pofd=pofd, roc_area=area)
