"""The NumPy restatement of include/radargrid_hydro.h: the texture along the ray and the table-driven fuzzy-logic classifier, each
in two forms -- a naive one that walks gate by gate with Python integers and floats, following the header line by line, and a
vectorised one that the GPU tests compare against.  tests/test_hydro_oracle.py holds the two equal to each other.  Nothing here
imports the package: the table arrives as plain arrays (``Spec``)."""
from typing import NamedTuple, Optional

import numpy as np

NAN_BITS = 0x7FC00000
NAN32 = np.uint32(NAN_BITS).view(np.float32)
MAX_ABS = 8192.0
SHIFT = 1024.0


class Texture(NamedTuple):
    sd: np.ndarray
    mean: np.ndarray
    count: np.ndarray


class Classes(NamedTuple):
    cls: np.ndarray          # uint8
    score: np.ndarray        # float32, NaN where cls == 0
    second: np.ndarray       # uint8
    best: np.ndarray         # float64: the best score before the thresholds (-1 where nothing was scored); not an output


class Spec(NamedTuple):
    """The table as the C ABI takes it."""
    kinds: tuple             # V values, 0 additive, 1 multiplicative
    required_bits: int
    cond_var: int
    edges: tuple             # B - 1 doubles
    cells: np.ndarray        # float64 [B][C][V][6]
    weights: np.ndarray      # float64 [C][V]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def compile_cells(vertices):
    """[..., 4] -> [..., 6]: the vertices rounded to float32 and back, r = 1 / (x2 - x1) where x2 > x1 and both are finite, else
    0; f likewise from x3 and x4."""
    with np.errstate(over="ignore"):
        v = np.asarray(vertices, np.float64).astype(np.float32).astype(np.float64)
    out = np.zeros(v.shape[:-1] + (6,))
    out[..., :4] = v
    flat_v, flat_o = v.reshape(-1, 4), out.reshape(-1, 6)
    for k in range(flat_v.shape[0]):
        x1, x2, x3, x4 = (float(t) for t in flat_v[k])
        flat_o[k, 4] = 1.0 / (x2 - x1) if np.isfinite(x1) and np.isfinite(x2) and x2 > x1 else 0.0
        flat_o[k, 5] = 1.0 / (x4 - x3) if np.isfinite(x3) and np.isfinite(x4) and x4 > x3 else 0.0
    return out


# ---- texture -----------------------------------------------------------------------------------------------------------------
def valid(x, mask=None):
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(x) & (np.abs(x) <= np.float32(MAX_ABS))
    return ok if mask is None else ok & (np.asarray(mask) == 0)


def fixed(x, ok):
    """q = llrint(1024 * (double)x) at the valid gates (ties to even), 0 elsewhere; int64."""
    return np.where(ok, np.rint(SHIFT * np.where(ok, x, np.float32(0)).astype(np.float64)), 0.0).astype(np.int64)


def texture_naive(x, mask, half_gates, min_valid, centre_only) -> Texture:
    x = np.asarray(x, np.float32)
    R, G = x.shape
    ok = valid(x, mask)
    q = fixed(x, ok)
    sd, mean = np.full((R, G), NAN32, np.float32), np.full((R, G), NAN32, np.float32)
    count = np.zeros((R, G), np.uint16)
    for r in range(R):
        for i in range(G):
            N = Sq = Sqq = 0                                             # Python integers: exact
            for j in range(max(0, i - half_gates), min(G - 1, i + half_gates) + 1):
                if ok[r, j]:
                    N += 1
                    Sq += int(q[r, j])
                    Sqq += int(q[r, j]) * int(q[r, j])
            count[r, i] = N
            if N >= min_valid and (not centre_only or ok[r, i]):
                D = N * Sqq - Sq * Sq
                assert 0 <= D < 2 ** 60 and N * Sqq < 2 ** 60 and Sq * Sq < 2 ** 60
                sd[r, i] = np.float32((np.sqrt(np.float64(D)) / np.float64(N)) / 1024.0)
                mean[r, i] = np.float32((np.float64(Sq) / np.float64(N)) / 1024.0)
    return Texture(sd, mean, count)


def texture(x, mask, half_gates, min_valid, centre_only) -> Texture:
    x = np.asarray(x, np.float32)
    R, G = x.shape
    ok = valid(x, mask)
    q = fixed(x, ok)

    def prefix(a):
        return np.concatenate([np.zeros((R, 1), np.int64), np.cumsum(a, axis=1, dtype=np.int64)], axis=1)
    i = np.arange(G)
    lo, hi = np.maximum(0, i - half_gates), np.minimum(G, i + half_gates + 1)
    pn, pq, pqq = prefix(ok.astype(np.int64)), prefix(q), prefix(q * q)
    N, Sq, Sqq = pn[:, hi] - pn[:, lo], pq[:, hi] - pq[:, lo], pqq[:, hi] - pqq[:, lo]
    D = N * Sqq - Sq * Sq
    defined = (N >= min_valid) & (ok if centre_only else True)
    n = np.where(defined, N, 1).astype(np.float64)
    sd = np.where(defined, ((np.sqrt(np.where(defined, D, 0).astype(np.float64)) / n) / 1024.0).astype(np.float32), NAN32)
    mean = np.where(defined, ((Sq.astype(np.float64) / n) / 1024.0).astype(np.float32), NAN32)
    return Texture(sd.astype(np.float32), mean.astype(np.float32), N.astype(np.uint16))


# ---- classifier --------------------------------------------------------------------------------------------------------------
def _membership_naive(x, cell):
    x1, x2, x3, x4, r, f = (float(t) for t in cell)
    if x < x1 or x > x4:
        return 0.0
    if x2 <= x <= x3:
        return 1.0
    with np.errstate(invalid="ignore", over="ignore"):
        t = float(np.float64(x - x1) * np.float64(r)) if x < x2 else float(np.float64(x4 - x) * np.float64(f))
    return t if t < 1.0 else 1.0


def classify_naive(variables, per_sweep_bits, rays_per_sweep, mask, spec: Spec, min_score) -> Classes:
    """The header, gate by gate.  The winner and the runner-up are found as the header DEFINES them: the largest score, the
    lowest class among equals; then the same among the other classes."""
    V = len(variables)
    B, C = spec.cells.shape[:2]
    shape = next(np.asarray(a).shape for v, a in enumerate(variables) if not (per_sweep_bits >> v) & 1)
    R, G = shape
    cls, second = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    score, best_out = np.full(shape, NAN32, np.float32), np.full(shape, -1.0)
    for ray in range(R):
        for g in range(G):
            value = [np.float32(variables[v][ray // rays_per_sweep if (per_sweep_bits >> v) & 1 else ray][g]) for v in range(V)]
            present = [bool(np.isfinite(t)) for t in value]
            if mask is not None and mask[ray][g] != 0:
                continue
            if any((spec.required_bits >> v) & 1 and not present[v] for v in range(V)):
                continue
            b = 0
            if spec.cond_var >= 0:
                if not present[spec.cond_var]:
                    continue
                b = sum(1 for e in spec.edges if value[spec.cond_var] >= np.float32(e))
            scores = []
            for c in range(C):
                A, W, P = 0.0, 0.0, 1.0
                for v in range(V):
                    if not present[v]:
                        continue
                    m = _membership_naive(float(value[v]), spec.cells[b, c, v])
                    if spec.kinds[v]:
                        P = P * m
                    else:
                        w = float(spec.weights[c, v])
                        A = A + w * m
                        W = W + w
                scores.append((A / W if W > 0.0 else 0.0) * P)
            numbers = [c for c in range(C) if scores[c] == scores[c]]
            if not numbers:
                continue
            k1 = min(numbers, key=lambda c: (-scores[c], c))
            best = scores[k1]
            best_out[ray, g] = best
            if not best > 0.0 or best < min_score:
                continue
            cls[ray, g] = k1 + 1
            score[ray, g] = np.float32(best)
            others = [c for c in numbers if c != k1]
            if others:
                second[ray, g] = min(others, key=lambda c: (-scores[c], c)) + 1
    return Classes(cls, score, second, best_out)


def memberships(x, cell):
    """x float64 [...], cell float64 [..., 6] -> the membership, float64."""
    x1, x2, x3, x4, r, f = (cell[..., k] for k in range(6))
    with np.errstate(invalid="ignore", over="ignore"):
        up, down = (x - x1) * r, (x4 - x) * f
        up, down = np.where(up < 1.0, up, 1.0), np.where(down < 1.0, down, 1.0)
        return np.where((x < x1) | (x > x4), 0.0, np.where((x2 <= x) & (x <= x3), 1.0, np.where(x < x2, up, down)))


def expand(variables, per_sweep_bits, rays_per_sweep):
    """Every variable as float32 [R][G]: the rows of a per-sweep table repeated for the rays of their sweep."""
    return [np.repeat(np.asarray(a, np.float32), rays_per_sweep, axis=0) if (per_sweep_bits >> v) & 1 else np.asarray(a, np.float32)
            for v, a in enumerate(variables)]


def classify(variables, per_sweep_bits, rays_per_sweep, mask, spec: Spec, min_score) -> Classes:
    """Vectorised; winner and runner-up in ONE pass over the classes, as the kernel does it."""
    full = expand(variables, per_sweep_bits, rays_per_sweep)
    V, shape = len(full), full[0].shape
    B, C = spec.cells.shape[:2]
    present = [np.isfinite(a) for a in full]
    classified = np.ones(shape, bool) if mask is None else np.asarray(mask) == 0
    for v in range(V):
        if (spec.required_bits >> v) & 1:
            classified &= present[v]
    bin_ = np.zeros(shape, np.int64)
    if spec.cond_var >= 0:
        classified &= present[spec.cond_var]
        with np.errstate(invalid="ignore"):
            for e in spec.edges:
                bin_ += full[spec.cond_var] >= np.float32(e)
    x = [np.where(present[v], full[v], np.float32(0)).astype(np.float64) for v in range(V)]
    best, nxt = np.full(shape, -1.0), np.full(shape, -1.0)
    k1, k2 = np.full(shape, -1, np.int64), np.full(shape, -1, np.int64)
    for c in range(C):
        A, W, P = np.zeros(shape), np.zeros(shape), np.ones(shape)
        for v in range(V):
            m = memberships(x[v], spec.cells[bin_, c, v])
            if spec.kinds[v]:
                P = np.where(present[v], P * m, P)
            else:
                w = float(spec.weights[c, v])
                A = np.where(present[v], A + w * m, A)
                W = np.where(present[v], W + w, W)
        with np.errstate(invalid="ignore", divide="ignore"):
            s = np.where(W > 0.0, A / np.where(W > 0.0, W, 1.0), 0.0) * P
            first = s > best
            runner = ~first & (s > nxt)
        nxt, k2 = np.where(first, best, np.where(runner, s, nxt)), np.where(first, k1, np.where(runner, c, k2))
        best, k1 = np.where(first, s, best), np.where(first, c, k1)
    best = np.where(classified, best, -1.0)
    won = classified & (k1 >= 0) & (best > 0.0) & ~(best < min_score)
    cls = np.where(won, k1 + 1, 0).astype(np.uint8)
    with np.errstate(invalid="ignore"):
        score = np.where(won, best.astype(np.float32), NAN32).astype(np.float32)
    second = np.where(won, k2 + 1, 0).astype(np.uint8)
    return Classes(cls, score, second, best)


# ---- the chain ---------------------------------------------------------------------------------------------------------------
def hydrometeors(dbz, zdr, kdp, rhohv, phidp, temperature, rays_per_sweep, mask, spec: Spec, half_gates=(2, 4),
                 min_valid=(3, 5), min_score=0.0):
    """classify_hydrometeors_device restated: two textures, then the classifier over (Z, ZDR, KDP, RHOHV, SD(Z), SD(PHIDP), T)
    with T per sweep; an absent variable is NaN everywhere.  -> (Classes, sd_dbz, sd_phidp or None)."""
    shape = dbz.shape
    absent = np.full(shape, NAN32, np.float32)
    sd_z = texture(dbz, mask, half_gates[0], min_valid[0], 0).sd
    sd_p = None if phidp is None else texture(phidp, mask, half_gates[1], min_valid[1], 0).sd
    t = np.full((shape[0] // rays_per_sweep, shape[1]), NAN32, np.float32) if temperature is None else temperature
    fields = [dbz, absent if zdr is None else zdr, absent if kdp is None else kdp, rhohv, sd_z, absent if sd_p is None else sd_p, t]
    return classify(fields, 1 << 6, rays_per_sweep, mask, spec, min_score), sd_z, sd_p


def spec_of(table) -> Spec:
    """The plain arrays of a ``MembershipTable`` (duck-typed: nothing is imported)."""
    return Spec(tuple(table.kinds), int(table.required_bits), int(table.cond_var), tuple(table.edges), np.asarray(table.cells),
                np.asarray(table.weights))
