"""The polar-domain phase processing restated in NumPy for the tests of ``radar_processor_amd/phase.py`` and
``csrc/rg_phase.hip`` -- written from the formulas of ``include/radargrid_phase.h``, never from either.  Sums are int64 (exact),
float32 and float64 stand exactly where the header puts them; every missing value is the quiet NaN ``0x7FC00000``.

``fit`` forms its sums through prefixes (vectorised: it also serves as the NumPy side of the timing); ``fit_direct`` forms them
gate by gate with Python integers.  Both must give the same bits: that is the point of the fixed point."""
from typing import NamedTuple, Optional

import numpy as np

NAN32 = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
MAX_ABS_PHI = 16384.0


class Fit(NamedTuple):
    kdp: np.ndarray
    phi_s: np.ndarray
    count: np.ndarray


class Attenuation(NamedTuple):
    dbz: np.ndarray
    zdr: Optional[np.ndarray]
    pia: np.ndarray
    dphi: np.ndarray


def bits(a):
    """The int32 bit patterns of a float32 array (NaN payloads count); other dtypes as they are."""
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


# ---- 1 unfold ------------------------------------------------------------------------------------------------------------------
def unfold(phidp, mask=None, wrap=360.0):
    """``(out float32, folds int32)``."""
    phidp = np.asarray(phidp, np.float32)
    R, G = phidp.shape
    valid = np.isfinite(phidp) if mask is None else np.isfinite(phidp) & (np.asarray(mask) == 0)
    half = np.float32(0.5 * float(wrap))
    out = np.full((R, G), NAN32, np.float32)
    folds = np.zeros((R, G), np.int32)
    for r in range(R):
        idx = np.flatnonzero(valid[r])
        if idx.size == 0:
            continue
        v = phidp[r, idx]
        d = v[1:] - v[:-1]                                             # float32
        k = np.zeros(idx.size, np.int64)
        k[1:] = np.where(d > half, -1, np.where(d < -half, 1, 0))
        K = np.cumsum(k)
        out[r, idx] = (v.astype(np.float64) + K.astype(np.float64) * float(wrap)).astype(np.float32)
        folds[r, idx] = K
    return out, folds


# ---- 2 fit ---------------------------------------------------------------------------------------------------------------------
def half_windows(dbz, shape, edges, half_window):
    """int64 [R, G]: the half-window of every gate."""
    hw = np.asarray(half_window, np.int64).reshape(-1)
    cls = np.zeros(shape, np.int64)
    if dbz is not None:
        z = np.asarray(dbz, np.float32)
        with np.errstate(invalid="ignore"):
            for e in edges:
                cls += z >= np.float32(e)                              # a NaN counts no edge
    return hw[cls]


def _fixed(phi):
    phi = np.asarray(phi, np.float32)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(phi) & (np.abs(phi) <= np.float32(MAX_ABS_PHI))
    q = np.zeros(phi.shape, np.int64)
    q[valid] = np.rint(65536.0 * phi[valid].astype(np.float64)).astype(np.int64)
    return valid, q


def _finish(N, Sj, Sjj, Sq, Sjq, centre, min_valid, centre_only, scale):
    den = N * Sjj - Sj * Sj
    num = N * Sjq - Sj * Sq
    defined = (N >= min_valid) & (den > 0)
    if centre_only:
        defined &= centre
    kdp = np.full(N.shape, NAN32, np.float32)
    phi_s = np.full(N.shape, NAN32, np.float32)
    s = num[defined].astype(np.float64) / den[defined].astype(np.float64)
    kdp[defined] = (s * float(scale)).astype(np.float32)
    phi_s[defined] = (((Sq[defined].astype(np.float64) - s * Sj[defined].astype(np.float64)) / N[defined].astype(np.float64))
                      / 65536.0).astype(np.float32)
    return Fit(kdp, phi_s, N.astype(np.uint16))


def fit(phi, scale, *, half_window=(15,), min_valid=2, dbz=None, edges=(), centre_only=False):
    """Sums through row-absolute int64 prefixes, re-centred on the gate: every term is an exact integer."""
    valid, q = _fixed(phi)
    R, G = valid.shape
    L = half_windows(dbz, (R, G), edges, half_window)
    x = np.arange(G, dtype=np.int64)[None, :]

    def prefix(a):
        return np.concatenate([np.zeros((R, 1), np.int64), np.cumsum(a, axis=1, dtype=np.int64)], axis=1)

    v = valid.astype(np.int64)
    P = [prefix(a) for a in (v, v * x, v * x * x, q, x * q)]
    lo = np.maximum(x - L, 0)
    hi = np.minimum(x + L, G - 1) + 1
    N, Sx, Sxx, Sq, Sxq = (np.take_along_axis(p, hi, 1) - np.take_along_axis(p, lo, 1) for p in P)
    Sj = Sx - x * N
    Sjj = Sxx - 2 * x * Sx + x * x * N
    Sjq = Sxq - x * Sq
    return _finish(N, Sj, Sjj, Sq, Sjq, valid, int(min_valid), bool(centre_only), scale)


def fit_direct(phi, scale, *, half_window=(15,), min_valid=2, dbz=None, edges=(), centre_only=False):
    """The same contract gate by gate, with Python integers and direct sums over the window."""
    valid, q = _fixed(phi)
    R, G = valid.shape
    L = half_windows(dbz, (R, G), edges, half_window)
    sums = np.zeros((5, R, G), np.int64)
    for r in range(R):
        for i in range(G):
            N = Sj = Sjj = Sq = Sjq = 0
            for g in range(max(0, i - int(L[r, i])), min(G - 1, i + int(L[r, i])) + 1):
                if valid[r, g]:
                    j, qq = g - i, int(q[r, g])
                    N, Sj, Sjj, Sq, Sjq = N + 1, Sj + j, Sjj + j * j, Sq + qq, Sjq + j * qq
            assert abs(N * Sjq) < 2 ** 57 and abs(Sj * Sq) < 2 ** 57
            sums[:, r, i] = (N, Sj, Sjj, Sq, Sjq)
    return _finish(*sums, valid, int(min_valid), bool(centre_only), scale)


# ---- 3 attenuation -------------------------------------------------------------------------------------------------------------
def attenuation(phi_s, dbz, *, alpha, beta, max_dphi, zdr=None, phi0=None):
    phi_s = np.asarray(phi_s, np.float32)
    dbz = np.asarray(dbz, np.float32)
    R, G = phi_s.shape
    cap = np.float32(max_dphi)
    m = np.zeros((R, G), np.float32)
    for r in range(R):
        origin = NAN32 if phi0 is None else np.float32(phi0[r])
        if np.isnan(origin):
            defined = np.flatnonzero(~np.isnan(phi_s[r]))
            if defined.size == 0:
                continue                                               # m = 0 everywhere
            origin = phi_s[r, defined[0]]
        with np.errstate(invalid="ignore"):
            e = phi_s[r] - origin                                      # float32
            e = np.where(e > 0, e, np.float32(0.0)).astype(np.float32)  # NaN, -0 and everything below count as +0
        m[r] = np.minimum(np.maximum.accumulate(e), cap)
    pia = (float(alpha) * m.astype(np.float64)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        out = dbz + pia
        zout = None if zdr is None else np.asarray(zdr, np.float32) + (float(beta) * m.astype(np.float64)).astype(np.float32)
    return Attenuation(out, zout, pia, m)
