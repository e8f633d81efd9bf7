"""NumPy / plain-Python restatement of include/radargrid_velocity.h, written from the header's formulas and from nothing else:
the bands, a flood-fill labelling with raster-order numbering per plane, the region edges, the greedy merge as a naive scan per
step (the product uses a heap and a union-find) and the apply.  Every decision rests on integers, so the tests hold the device
outputs EQUAL to these."""
from typing import NamedTuple

import numpy as np

MAX_ABS = 16384.0
QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def bits(a):
    """The array's own bits as unsigned integers: equality that tells NaN payloads and -0 from +0."""
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def as_volume(vel):
    vel = np.asarray(vel)
    return vel[None] if vel.ndim == 2 else vel


def nyquists(nyquist, S):
    v = np.asarray(nyquist, np.float64)
    return np.full(S, float(v)) if v.ndim == 0 else v


def valid(v, mask=None):
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(v) & (np.abs(v) <= np.float32(MAX_ABS))
    return ok if mask is None else ok & (np.asarray(mask) == 0)


def fixed(v):
    """q = llrint(65536 * (double)v) where v is valid, 0 elsewhere."""
    v = np.asarray(v)
    return np.rint(65536.0 * np.where(valid(v), v, np.float32(0)).astype(np.float64)).astype(np.int64)


def interval(vn):
    return int(np.rint(65536.0 * 2.0 * float(vn)))


def bands(vel, nyquist, B, mask=None):
    """int64 [S][R][G]: the band of every valid gate, -1 elsewhere."""
    vel = as_volume(vel)
    vn = nyquists(nyquist, vel.shape[0])[:, None, None]
    ok = valid(vel, None if mask is None else as_volume(mask))
    v = np.where(ok, vel, np.float32(0)).astype(np.float64)
    t = np.floor((v + vn) * B / (2.0 * vn))
    return np.where(ok, np.clip(t, 0, B - 1).astype(np.int64), -1)


def split(vel, nyquist, B, mask=None):
    vel = as_volume(vel)
    band = bands(vel, nyquist, B, mask)
    out = np.full((vel.shape[0], B) + vel.shape[1:], QNAN, np.float32)
    for b in range(B):
        out[:, b][band == b] = vel[band == b]
    return out


def label_plane(fg, wrap):
    """4-connected flood fill of the boolean plane; cells numbered from 1 in raster order of their first pixel."""
    h, w = fg.shape
    labels = np.zeros((h, w), np.int32)
    n = 0
    for y0, x0 in zip(*np.nonzero(fg)):
        if labels[y0, x0]:
            continue
        n += 1
        labels[y0, x0] = n
        stack = [(int(y0), int(x0))]
        while stack:
            y, x = stack.pop()
            for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                if wrap:
                    yy %= h
                if 0 <= yy < h and 0 <= xx < w and fg[yy, xx] and not labels[yy, xx]:
                    labels[yy, xx] = n
                    stack.append((yy, xx))
    return labels, n


class Regions(NamedTuple):
    regions: np.ndarray      # int32 [S][R][G], 0 = none, ids from 1
    sizes: np.ndarray        # int32 [n]
    cell_ptr: np.ndarray     # int32 [S * B + 1]
    labels: np.ndarray       # int32 [S][B][R][G]


def regions(vel, nyquist, B, mask=None, wrap=True):
    vel = as_volume(vel)
    S = vel.shape[0]
    band = bands(vel, nyquist, B, mask)
    out = np.zeros(vel.shape, np.int32)
    labels = np.zeros((S, B) + vel.shape[1:], np.int32)
    ptr = [0]
    for s in range(S):
        for b in range(B):
            lab, n = label_plane(band[s] == b, wrap)
            labels[s, b] = lab
            out[s][lab > 0] = ptr[-1] + lab[lab > 0]
            ptr.append(ptr[-1] + n)
    sizes = np.bincount(out.reshape(-1), minlength=ptr[-1] + 1)[1:].astype(np.int32)
    return Regions(out, sizes, np.array(ptr, np.int32), labels)


def flatten(labels, cell_ptr, B):
    """rg_velocity_regions_i32 for any labels [S][B][R][G]: the lowest band whose label is > 0 and within its plane's count."""
    S = labels.shape[0]
    out = np.zeros((S,) + labels.shape[2:], np.int32)
    for s in range(S):
        for b in reversed(range(B)):
            p = s * B + b
            lab = labels[s, b].astype(np.int64)
            ok = (lab > 0) & (lab <= int(cell_ptr[p + 1]) - int(cell_ptr[p]))
            out[s][ok] = (int(cell_ptr[p]) + lab[ok]).astype(np.int32)
    return out


def edges(values, region, wrap):
    """int64 [n][4]: (lo, hi, count, sum) sorted by (lo, hi), over planes [n_planes][h][w]."""
    values, region = as_volume(values), as_volume(region)
    n, h, w = values.shape
    q, ok = fixed(values), valid(values) & (region > 0)
    found = {}

    def pair(a, b):                                  # a, b: index tuples of the pixel and its forward neighbour
        ra, rb = region[a].astype(np.int64), region[b].astype(np.int64)
        use = ok[a] & ok[b] & (ra != rb)
        lo, hi = np.minimum(ra, rb)[use], np.maximum(ra, rb)[use]
        d = np.where(ra < rb, q[b] - q[a], q[a] - q[b])[use]
        for l, hh, dd in zip(lo.tolist(), hi.tolist(), d.tolist()):
            c = found.setdefault((l, hh), [0, 0])
            c[0] += 1
            c[1] += dd

    if w > 1:
        pair(np.s_[:, :, :-1], np.s_[:, :, 1:])
    if h > 1:
        pair(np.s_[:, :-1, :], np.s_[:, 1:, :])
    if wrap and h >= 3:
        pair(np.s_[:, h - 1, :], np.s_[:, 0, :])
    return np.array([[lo, hi, c, s] for (lo, hi), (c, s) in sorted(found.items())], np.int64).reshape(-1, 4)


def merge(edge_rows, sizes, intervals):
    """The merge of the header, as a scan over all edges per step.  Returns the int64 fold of every region."""
    n = len(sizes)
    sizes = [int(v) for v in sizes]
    members = {k + 1: [k + 1] for k in range(n)}     # set id (its smallest region id) -> region ids
    fold = {k + 1: 0 for k in range(n)}
    table = {(int(lo), int(hi)): [int(c), int(s)] for lo, hi, c, s in np.asarray(edge_rows, dtype=object).reshape(-1, 4).tolist()}
    while table:
        (lo, hi), (c, s) = min(table.items(), key=lambda kv: (-kv[1][0], kv[0]))
        g_lo, g_hi = sum(sizes[r - 1] for r in members[lo]), sum(sizes[r - 1] for r in members[hi])
        if g_lo >= g_hi:
            base, m, s_mb = lo, hi, s                # s is oriented hi - lo = M - base
        else:
            base, m, s_mb = hi, lo, -s
        big_i = intervals[m - 1]
        w = c * big_i
        k = (2 * s_mb + w) // (2 * w)
        for r in members[m]:
            fold[r] -= k
        del table[(lo, hi)]
        moved = {}
        for (a, b), (cx, sx) in list(table.items()):
            if m not in (a, b):
                continue
            del table[(a, b)]
            x = b if a == m else a
            s_xm = sx if a == m else -sx             # oriented X - M
            moved[x] = (cx, s_xm + k * cx * big_i)
        name = min(base, m)
        members[name] = sorted(members.pop(base) + members.pop(m))
        renamed = {}
        for (a, b), cs in list(table.items()):       # the base's own edges, under the merged set's name
            if base in (a, b):
                del table[(a, b)]
                x = b if a == base else a
                renamed[x] = (cs[0], cs[1] if a == base else -cs[1])      # oriented X - base
        for x, (cx, sx) in moved.items():
            c0, s0 = renamed.get(x, (0, 0))
            renamed[x] = (c0 + cx, s0 + sx)
        for x, (cx, sx) in renamed.items():          # oriented X - merged set; the table keeps hi - lo
            table[(min(name, x), max(name, x))] = [cx, sx if name < x else -sx]
    out = np.zeros(n, np.int64)
    for regs in members.values():
        weight = {}
        for r in regs:
            weight[fold[r]] = weight.get(fold[r], 0) + sizes[r - 1]
        best = max(weight.values())
        centre = sorted((abs(f), f) for f, g in weight.items() if g == best)[0][1]
        for r in regs:
            out[r - 1] = fold[r] - centre
    return out


def region_intervals(cell_ptr, nyquist, B):
    S = (len(cell_ptr) - 1) // B
    vn = nyquists(nyquist, S)
    out = []
    for p in range(S * B):
        out += [interval(vn[p // B])] * (int(cell_ptr[p + 1]) - int(cell_ptr[p]))
    return out


def apply(vel, region, lut, nyquist):
    """(out float32, folds int32) of the volume's shape."""
    shape = np.asarray(vel).shape
    vel, region = as_volume(vel), as_volume(region)
    lut = np.asarray(lut, np.int64)
    vn = nyquists(nyquist, vel.shape[0])[:, None, None]
    ok = (region > 0) & (region <= len(lut))
    f = np.zeros(vel.shape, np.int64)
    f[ok] = lut[region[ok].astype(np.int64) - 1]
    with np.errstate(invalid="ignore", over="ignore"):
        out = (vel.astype(np.float64) + f.astype(np.float64) * (2.0 * vn)).astype(np.float32)
    bad = ~ok | np.isnan(out)
    out[bad] = QNAN
    f[bad] = 0
    return out.reshape(shape), f.astype(np.int32).reshape(shape)


class Dealiased(NamedTuple):
    velocity: np.ndarray
    folds: np.ndarray
    regions: np.ndarray
    n_regions: int
    edges: np.ndarray
    lut: np.ndarray


def dealias(vel, nyquist, B=3, mask=None, wrap=True):
    shape = np.asarray(vel).shape
    reg = regions(vel, nyquist, B, mask, wrap)
    e = edges(as_volume(vel), reg.regions, wrap)
    lut = merge(e, reg.sizes, region_intervals(reg.cell_ptr, nyquist, B))
    out, folds = apply(as_volume(vel), reg.regions, lut, nyquist)
    return Dealiased(out.reshape(shape), folds.reshape(shape), reg.regions.reshape(shape), len(reg.sizes), e, lut)
