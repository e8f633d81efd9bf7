"""The NumPy restatement of include/radargrid_shear.h: what the kernels of csrc/rg_shear.hip are held EQUAL to.

``moments`` forms the nine window sums as int64 planes from shifted, masked copies of the volume -- a loop over the (i, j)
offsets of the window, ``np.roll`` along the rays for the wrap; the five sums of one ray offset are formed over j and added with
the weights 1, i, i * i where the centre gate's half-width reaches i -- and ``llsd`` applies the header's formulas in float64, in the
header's order.  ``median`` sorts the window stack.  ``llsd_naive`` and ``median_naive`` do the same gate by gate in Python
ints and floats, for tiny shapes: the two restatements check each other (tests/test_shear_oracle.py)."""
from typing import NamedTuple

import numpy as np

MAX_ABS = 16384.0
NAN_BITS = np.uint32(0x7FC00000)
NAN32 = np.array([NAN_BITS], np.uint32).view(np.float32)[0]


class Llsd(NamedTuple):
    az_shear: np.ndarray
    divergence: np.ndarray
    vel_s: np.ndarray
    count: np.ndarray


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def as_volume(a):
    a = np.asarray(a)
    return a[None] if a.ndim == 2 else a


def valid(vel, mask=None):
    vel = as_volume(vel)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(vel) & (np.abs(vel) <= np.float32(MAX_ABS))
    if mask is not None:
        ok &= as_volume(mask) == 0
    return ok


def fixed_point(vel, ok):
    """q = llrint(65536 * (double)v) where valid, 0 elsewhere."""
    return np.rint(65536.0 * np.where(ok, as_volume(vel), 0).astype(np.float64)).astype(np.int64)


def clamp_half(half_rays, max_half_rays):
    return np.clip(np.asarray(half_rays, dtype=np.int64), 0, int(max_half_rays))


def _shift_rays(a, i, wrap):
    """out[:, r] = a[:, r + i]; rays outside the sweep are ray (r + i) mod R with ``wrap``, absent (zero) without."""
    if wrap:
        return np.roll(a, -i, axis=1)
    out = np.zeros_like(a)
    R = a.shape[1]
    lo, hi = max(0, -i), min(R, R - i)
    if lo < hi:
        out[:, lo:hi] = a[:, lo + i:hi + i]
    return out


NAMES = ("n", "Si", "Sj", "Sii", "Sij", "Sjj", "Sq", "Siq", "Sjq")


def moments(vel, mask, half_rays, max_half_rays, half_gates, wrap):
    """The nine sums of every gate's window, int64 ``[S, R, G]`` each, and the validity plane."""
    ok = valid(vel, mask)
    q = fixed_point(vel, ok)
    S, R, G = ok.shape
    ka = clamp_half(half_rays, max_half_rays)
    m = {name: np.zeros((S, R, G), np.int64) for name in NAMES}
    part = {name: np.zeros((S, R, G), np.int64) for name in ("n", "Sj", "Sjj", "Sq", "Sjq")}
    for i in range(-int(ka.max(initial=0)), int(ka.max(initial=0)) + 1):
        ok_i = _shift_rays(ok, i, wrap).astype(np.int64)
        q_i = _shift_rays(q, i, wrap)                                              # 0 where not valid
        for plane in part.values():
            plane[...] = 0
        for j in range(-half_gates, half_gates + 1):
            lo, hi = max(0, -j), min(G, G - j)                                     # centre gates whose gate g + j exists
            if lo >= hi:
                continue
            w, wq = ok_i[:, :, lo + j:hi + j], q_i[:, :, lo + j:hi + j]
            dst = (slice(None), slice(None), slice(lo, hi))
            part["n"][dst] += w
            part["Sj"][dst] += j * w
            part["Sjj"][dst] += j * j * w
            part["Sq"][dst] += wq
            part["Sjq"][dst] += j * wq
        use = (ka >= abs(i)).astype(np.int64)[None, None, :]                       # the CENTRE gate's half-width decides
        m["n"] += use * part["n"]
        m["Si"] += use * (i * part["n"])
        m["Sj"] += use * part["Sj"]
        m["Sii"] += use * (i * i * part["n"])
        m["Sij"] += use * (i * part["Sj"])
        m["Sjj"] += use * part["Sjj"]
        m["Sq"] += use * part["Sq"]
        m["Siq"] += use * (i * part["Sq"])
        m["Sjq"] += use * part["Sjq"]
    return m, ok


def normal_terms(m):
    n = m["n"]
    A = n * m["Sii"] - m["Si"] * m["Si"]
    B = n * m["Sij"] - m["Si"] * m["Sj"]
    C = n * m["Sjj"] - m["Sj"] * m["Sj"]
    P = n * m["Siq"] - m["Si"] * m["Sq"]
    Q = n * m["Sjq"] - m["Sj"] * m["Sq"]
    return A, B, C, P, Q, A * C - B * B


def defined_plane(m, ok, half_rays, max_half_rays, half_gates, min_valid, min_fraction_q16, centre_only):
    ka = clamp_half(half_rays, max_half_rays)
    W = (2 * ka + 1) * (2 * half_gates + 1)
    D = normal_terms(m)[5]
    defined = (m["n"] >= min_valid) & (m["n"] * 65536 >= int(min_fraction_q16) * W[None, None, :]) & (D > 0)
    if centre_only:
        defined &= ok
    return defined


def _quiet(x, defined):
    x = x.astype(np.float32)
    return np.where(defined & ~np.isnan(x), x, NAN32)


def llsd(vel, mask, half_rays, az_scale, max_half_rays, half_gates, range_scale, wrap, min_valid, min_fraction_q16, centre_only):
    m, ok = moments(vel, mask, half_rays, max_half_rays, half_gates, wrap)
    A, B, C, P, Q, D = normal_terms(m)
    defined = defined_plane(m, ok, half_rays, max_half_rays, half_gates, min_valid, min_fraction_q16, centre_only)
    f = np.float64
    with np.errstate(all="ignore"):
        Dd = np.where(defined, D, 1).astype(f)
        nd = np.where(defined, m["n"], 1).astype(f)
        al = (P.astype(f) * C.astype(f) - Q.astype(f) * B.astype(f)) / Dd
        be = (Q.astype(f) * A.astype(f) - P.astype(f) * B.astype(f)) / Dd
        shear = al * np.asarray(az_scale, f)[None, None, :]
        div = be * f(range_scale)
        smooth = (((m["Sq"].astype(f) - al * m["Si"].astype(f)) - be * m["Sj"].astype(f)) / nd) / 65536.0
        out = Llsd(_quiet(shear, defined), _quiet(div, defined), _quiet(smooth, defined), m["n"].astype(np.uint16))
    return out


def llsd_naive(vel, mask, half_rays, az_scale, max_half_rays, half_gates, range_scale, wrap, min_valid, min_fraction_q16,
               centre_only):
    """Gate by gate in Python ints (the sums) and Python floats (IEEE float64; ``float(int)`` rounds to nearest even)."""
    vel = as_volume(vel)
    ok = valid(vel, mask)
    S, R, G = vel.shape
    q = fixed_point(vel, ok).tolist()
    okl = ok.tolist()
    outs = [np.full((S, R, G), NAN32, np.float32) for _ in range(3)]
    count = np.zeros((S, R, G), np.uint16)
    for s in range(S):
        for a in range(R):
            for g in range(G):
                ka = min(max(int(half_rays[g]), 0), max_half_rays)
                n = Si = Sj = Sii = Sij = Sjj = Sq = Siq = Sjq = 0
                for i in range(-ka, ka + 1):
                    ai = a + i
                    if wrap:
                        ai %= R
                    elif not 0 <= ai < R:
                        continue
                    for j in range(-half_gates, half_gates + 1):
                        gj = g + j
                        if not 0 <= gj < G or not okl[s][ai][gj]:
                            continue
                        v = q[s][ai][gj]
                        n += 1; Si += i; Sj += j; Sii += i * i; Sij += i * j; Sjj += j * j   # noqa: E702
                        Sq += v; Siq += i * v; Sjq += j * v                                    # noqa: E702
                count[s, a, g] = n
                A, B, C = n * Sii - Si * Si, n * Sij - Si * Sj, n * Sjj - Sj * Sj
                P, Q = n * Siq - Si * Sq, n * Sjq - Sj * Sq
                D = A * C - B * B
                W = (2 * ka + 1) * (2 * half_gates + 1)
                if n < min_valid or n * 65536 < min_fraction_q16 * W or D <= 0 or (centre_only and not okl[s][a][g]):
                    continue
                al = (float(P) * float(C) - float(Q) * float(B)) / float(D)
                be = (float(Q) * float(A) - float(P) * float(B)) / float(D)
                with np.errstate(all="ignore"):
                    res = (np.float32(np.float64(al) * np.float64(az_scale[g])), np.float32(np.float64(be) * np.float64(range_scale)),
                           np.float32((((float(Sq) - al * float(Si)) - be * float(Sj)) / float(n)) / 65536.0))
                for o, r in zip(outs, res):
                    o[s, a, g] = NAN32 if np.isnan(r) else r
    return Llsd(outs[0], outs[1], outs[2], count)


def median(vel, mask, half_rays, half_gates, wrap, min_valid, centre_only):
    """The lower median of the valid gates of every window, by sorting the window stack (+inf pads sort last)."""
    vel = as_volume(vel).astype(np.float32)
    ok = valid(vel, mask)
    S, R, G = vel.shape
    padded = np.where(ok, vel, np.float32(np.inf))
    stack = []
    for i in range(-half_rays, half_rays + 1):
        p_i = _shift_rays(padded, i, wrap)
        in_i = _shift_rays(np.ones_like(ok), i, wrap)
        p_i = np.where(in_i, p_i, np.float32(np.inf))
        for j in range(-half_gates, half_gates + 1):
            plane = np.full((S, R, G), np.inf, np.float32)
            lo, hi = max(0, -j), min(G, G - j)
            if lo < hi:
                plane[:, :, lo:hi] = p_i[:, :, lo + j:hi + j]
            stack.append(plane)
    stack = np.sort(np.stack(stack, axis=-1), axis=-1)
    n = np.isfinite(stack).sum(axis=-1)
    pick = np.take_along_axis(stack, (np.maximum(n - 1, 0) // 2)[..., None], axis=-1)[..., 0]
    keep = n >= min_valid
    if centre_only:
        keep &= ok
    return np.where(keep, pick, NAN32).astype(np.float32)


def median_naive(vel, mask, half_rays, half_gates, wrap, min_valid, centre_only):
    vel = as_volume(vel).astype(np.float32)
    ok = valid(vel, mask)
    S, R, G = vel.shape
    out = np.full((S, R, G), NAN32, np.float32)
    for s in range(S):
        for a in range(R):
            for g in range(G):
                values = []
                for i in range(-half_rays, half_rays + 1):
                    ai = a + i
                    if wrap:
                        ai %= R
                    elif not 0 <= ai < R:
                        continue
                    for j in range(-half_gates, half_gates + 1):
                        if 0 <= g + j < G and ok[s, ai, g + j]:
                            values.append(vel[s, ai, g + j])
                if len(values) >= min_valid and (ok[s, a, g] or not centre_only):
                    out[s, a, g] = sorted(values)[(len(values) - 1) // 2]
    return out
