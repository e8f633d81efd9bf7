"""Plain NumPy restatements and hand-made inputs for the prologue kernels every gridding path starts with
(``rg_pack_fields_f32``, ``rg_gate_mask_f32``, ``rg_scan_counts_i64``, ``rg_geom_bin_gates_f32`` and the per-level lists),
written from the contracts in include/radargrid_hip.h -- never from the kernels.  No GPU is needed here: what the
generators promise is asserted by tests/test_prologue_scenes.py, what the kernels do with them by
tests/test_gpu_prologue.py."""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import radar_grid_oracle as oracle

EXCLUDED_BITS = 0x7FD1CE5D          # RG_EXCLUDED_BITS
CANONICAL_NAN = 0x7FC00000
STRIDES = (1, 2, 4, 8)
GATE_OPS = ("below", "above", "between", "outside", "equal", "invalid")
F32 = np.float32
INF32 = F32(np.inf)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def from_bits(b) -> np.ndarray:
    return np.asarray(b, dtype=np.uint32).view(np.float32)


def strides_for(n_fields: int):
    """Every stride rg_pack_fields_f32 accepts for ``n_fields`` fields."""
    return tuple(s for s in STRIDES if s >= n_fields)


# ---- pack ------------------------------------------------------------------------------------------------------------------
def special_values() -> dict:
    """name -> float32 bit pattern of the values planted into packed fields."""
    return dict(pos_zero=0x00000000, neg_zero=0x80000000, pos_inf=0x7F800000, neg_inf=0xFF800000,
                denormal=0x00000001, neg_denormal=0x80000001, huge=int(bits([3.0e38])[0]),
                qnan=0x7FC00000, neg_qnan=0xFFC00000, payload_nan=0x7FC12345, neg_sentinel=0xFFD1CE5D,
                sentinel=EXCLUDED_BITS, snan=0x7F800001)


def is_signalling(b) -> np.ndarray:
    b = np.asarray(b, dtype=np.uint32)
    return ((b & 0x7F800000) == 0x7F800000) & ((b & 0x007FFFFF) != 0) & ((b & 0x00400000) == 0)


def _excluded(masks, shared, n_fields, n_gates):
    ex = np.zeros((n_gates, n_fields), dtype=bool)
    for f in range(n_fields):
        if masks is not None and masks[f] is not None:
            ex[:, f] |= np.asarray(masks[f]) != 0            # any non-zero byte counts
        if shared is not None:
            ex[:, f] |= np.asarray(shared) != 0
    return ex


def pack_fields_ref(fields, masks, shared, stride) -> np.ndarray:
    """uint32 bits of the packed ``[G][stride]`` layout: the sentinel in masked and padding slots, the value's own bits in
    unmasked ones.  An unmasked value that carries the sentinel's bits is stored as SOME NaN other than the sentinel: this
    array holds the canonical quiet NaN there, and :func:`pack_loose_slots` marks the slot as one whose exact bits the
    contract leaves open."""
    n_fields, n_gates = len(fields), len(fields[0])
    assert stride in STRIDES and stride >= n_fields
    out = np.full((n_gates, stride), EXCLUDED_BITS, dtype=np.uint32)
    ex = _excluded(masks, shared, n_fields, n_gates)
    for f in range(n_fields):
        b = bits(fields[f])
        b = np.where(b == EXCLUDED_BITS, np.uint32(CANONICAL_NAN), b)
        out[:, f] = np.where(ex[:, f], np.uint32(EXCLUDED_BITS), b)
    return out


def pack_loose_slots(fields, masks, shared, stride) -> np.ndarray:
    """bool ``[G][stride]``: unmasked slots whose value aliases the sentinel or is a signalling NaN -- the packed value
    must be a NaN that is not the sentinel; its payload is not prescribed."""
    n_fields, n_gates = len(fields), len(fields[0])
    loose = np.zeros((n_gates, stride), dtype=bool)
    ex = _excluded(masks, shared, n_fields, n_gates)
    for f in range(n_fields):
        b = bits(fields[f])
        loose[:, f] = ~ex[:, f] & ((b == EXCLUDED_BITS) | is_signalling(b))
    return loose


# ---- gate mask -------------------------------------------------------------------------------------------------------------
def _around(v):
    v = F32(v)
    return [v, np.nextafter(v, INF32), np.nextafter(v, -INF32)]


def _common_data():
    sp = special_values()
    vals = [from_bits([sp[k]])[0] for k in ("pos_zero", "neg_zero", "pos_inf", "neg_inf", "denormal", "neg_denormal", "huge",
                                           "qnan", "neg_qnan", "payload_nan", "sentinel", "snan")]
    rng = np.random.default_rng(5)
    return vals + list(rng.normal(0.4, 0.6, 40).astype(np.float32))


def _equal_data(a, b):
    """The float32 lattice around a + b and a - b, eight steps each way: the values d whose fl32(|d - a|) is nearest to
    fl32(b) on either side, and equal to it where the lattice allows (with a = 0 the difference is |d| itself: exactly b and
    one ulp either side).  The subtraction is evaluated in float32, as the kernel and the oracle do."""
    a32, b32 = F32(a), F32(b)
    out = []
    for centre in (a32 + b32, a32 - b32):
        d = [centre]
        lo = hi = centre
        for _ in range(8):
            lo, hi = np.nextafter(lo, -INF32), np.nextafter(hi, INF32)
            d += [lo, hi]
        out += d
    return out


def gate_mask_cases():
    """``[(op, a, b, data float32)]`` for the six GateFilter predicates.  ``a`` / ``b`` are Python floats, several of them
    not float32 values (0.1, 0.8): the C ABI rounds them to float32, the reference is ``oracle.gate_mask`` with
    ``np.float32`` thresholds (:func:`gate_mask_ref`).  Every data array holds the thresholds, their float32 neighbours on
    both sides, +-0, +-inf, NaNs, denormals and a few ordinary numbers."""
    pairs = {
        "below": [(0.0, 0.0), (0.8, 0.0), (0.1, 0.0), (-3.5, 0.0), (1.4e-45, 0.0)],
        "above": [(0.0, 0.0), (0.8, 0.0), (0.1, 0.0), (-3.5, 0.0), (-1.4e-45, 0.0)],
        "between": [(0.1, 0.8), (0.0, 1.0), (-0.0, 0.0), (2.0, 2.0), (-1.0, 3.0e38)],
        "outside": [(0.1, 0.8), (0.0, 1.0), (-0.0, 0.0), (2.0, 2.0), (0.8, 0.1)],
        "equal": [(0.8, 0.1), (1.0, 0.5), (0.0, 0.8), (0.0, 1.4e-45), (0.1, 0.0), (-3.5, 0.8)],
        "invalid": [(0.0, 0.0)],
    }
    cases = []
    for op in GATE_OPS:
        for a, b in pairs[op]:
            d = _common_data() + _around(a) + _around(b)
            if op == "equal":
                d += _equal_data(a, b)
            cases.append((op, a, b, np.array(d, dtype=np.float32)))
    return cases


def gate_mask_ref(op, data, a, b) -> np.ndarray:
    return oracle.gate_mask(op, np.asarray(data, dtype=np.float32), np.float32(a), np.float32(b))


def tile_to(data, n) -> np.ndarray:
    return np.resize(np.asarray(data, dtype=np.float32), n)


# ---- the gate lists --------------------------------------------------------------------------------------------------------
def make_cells(x0, y0, cell, ncx, ncy, z_lo, z_hi):
    return SimpleNamespace(x0=float(x0), y0=float(y0), inv_cx=1.0 / float(cell), inv_cy=1.0 / float(cell), z_lo=float(z_lo),
                           z_hi=float(z_hi), ncx=int(ncx), ncy=int(ncy), cell=float(cell))


def gate_cells(gx, gy, gz, alt, toa, cells):
    """``(z_rel float32, keep bool, cell int64)`` of every gate: the keep rule and the cell key of the header, in float64,
    operation by operation.  NaN fails every comparison; +-inf fails a range test."""
    gx, gy, gz = (np.asarray(v, dtype=np.float32) for v in (gx, gy, gz))
    with np.errstate(invalid="ignore", over="ignore"):
        z_rel = (gz - F32(alt)).astype(np.float32)                      # float32 subtraction
        x, y, z = gx.astype(np.float64), gy.astype(np.float64), z_rel.astype(np.float64)
        tx = np.floor((x - cells.x0) * cells.inv_cx)
        ty = np.floor((y - cells.y0) * cells.inv_cy)
        keep = ((z_rel <= F32(toa)) & (z >= cells.z_lo) & (z <= cells.z_hi) & (tx >= 0.0) & (tx < cells.ncx) & (ty >= 0.0)
                & (ty < cells.ncy))
    cell = np.full(gx.shape, -1, dtype=np.int64)
    cell[keep] = ty[keep].astype(np.int64) * cells.ncx + tx[keep].astype(np.int64)
    return z_rel, keep, cell


RECORD = np.dtype([("x", "<u4"), ("y", "<u4"), ("z", "<u4"), ("index", "<i4")])       # rg_gate4, floats as their bits


def _records(gx, gy, z_rel, order) -> np.ndarray:
    rec = np.zeros(order.size, dtype=RECORD)
    rec["x"], rec["y"], rec["z"] = bits(gx)[order], bits(gy)[order], bits(z_rel)[order]
    rec["index"] = order
    return rec


def _starts(sorted_keys, n_keys) -> np.ndarray:
    return np.searchsorted(sorted_keys, np.arange(n_keys + 1), side="left").astype(np.int32)


def bin_gates_ref(gx, gy, gz, alt, toa, cells):
    """``(records, cell_start)`` of rg_geom_bin_gates_f32: the kept gates in (cell, gate index) order as (x, y, z_rel,
    index) records, ``cell_start[c]`` the first position whose cell is >= c, ``cell_start[ncx * ncy]`` = gates kept."""
    z_rel, keep, cell = gate_cells(gx, gy, gz, alt, toa, cells)
    kept = np.nonzero(keep)[0]
    order = kept[np.argsort(cell[kept], kind="stable")]
    return _records(gx, gy, z_rel, order), _starts(cell[order], cells.ncx * cells.ncy)


def level_lists_ref(gx, gy, gz, alt, toa, cells, zc, min_radius, beam_factor):
    """``(must, may, never)`` boolean ``[nz][G]``: a kept gate MUST be listed under level iz when ``|z_rel - zc[iz]| <= R_g``,
    ``R_g = max(min_radius, |g| * bf / (1 - bf))`` in float64; it MAY be listed up to the documented inflation
    ``(1 + 1e-6) * R_g + 1 mm`` (with 1e-12 relative slack for the order in which bf / (1 - bf) is formed); NEVER beyond, and
    never when the keep rule drops it."""
    z_rel, keep, _ = gate_cells(gx, gy, gz, alt, toa, cells)
    with np.errstate(invalid="ignore", over="ignore"):
        x, y, z = (np.asarray(gx, np.float32).astype(np.float64), np.asarray(gy, np.float32).astype(np.float64),
                   z_rel.astype(np.float64))
        norm = np.sqrt(x * x + y * y + z * z)
        r_g = np.maximum(float(min_radius), norm * float(beam_factor) / (1.0 - float(beam_factor)))
        dz = np.abs(z[None, :] - np.asarray(zc, dtype=np.float32).astype(np.float64)[:, None])
        must = keep[None, :] & (dz <= r_g[None, :])
        reach = (r_g * (1.0 + 1e-6) + 1e-3) * (1.0 + 1e-12)
        may = keep[None, :] & ~must & (dz <= reach[None, :])
    return must, may, ~(must | may)


def level_order_ref(gx, gy, gz, alt, toa, cells, listed):
    """``(records, cell_start)`` of rg_geom_bin_gates_levels_f32 for the (level, gate) set ``listed`` (bool ``[nz][G]``): the
    entries in (level, cell, gate index) order, ``cell_start[nz * ncx * ncy + 1]`` with level iz's cells at iz * ncx * ncy."""
    z_rel, keep, cell = gate_cells(gx, gy, gz, alt, toa, cells)
    assert not listed[:, ~keep].any()
    lev, gate = np.nonzero(listed)                                     # row-major: (level, gate index)
    key = lev.astype(np.int64) * (cells.ncx * cells.ncy) + cell[gate]
    order = np.argsort(key, kind="stable")
    return _records(gx, gy, z_rel, gate[order]), _starts(key[order], listed.shape[0] * cells.ncx * cells.ncy)


def _gz_for(z_rel_target, alt32):
    """A float32 height whose float32 difference to ``alt32`` is exactly ``z_rel_target``."""
    t = F32(z_rel_target)
    lo = hi = F32(np.float64(t) + np.float64(alt32))
    for _ in range(64):
        for g in (lo, hi):
            if F32(g - alt32) == t:
                return g
        lo, hi = np.nextafter(lo, -INF32), np.nextafter(hi, INF32)
    raise AssertionError(f"no float32 height gives z_rel = {t!r} above {alt32!r}")


# The planted cases of a binning scene -> (kept?, how many gates at least)
PLANTED = dict(x_boundary=(True, 6), x_below_boundary=(True, 6), y_boundary=(True, 2), y_below_boundary=(True, 2),
               x_at_origin=(True, 1), x_inside_origin=(True, 1), x_below_origin=(False, 1), x_at_end=(False, 1),
               x_inside_end=(True, 1), y_at_origin=(True, 1), y_inside_origin=(True, 1), y_below_origin=(False, 1),
               y_at_end=(False, 1), y_inside_end=(True, 1), z_at_top=(True, 2), z_above_top=(False, 2), z_at_lo=(True, 2),
               z_below_lo=(False, 2), nonfinite=(False, 9), duplicates=(True, 5))
CELL, X0, Y0, NCX, NCY = 1024.0, -4096.0, 1024.0, 7, 3
Z_LO, Z_HI = -512.0, 8192.0
EMPTY_MIDDLE = 1 * NCX + 3                    # cell (cx 3, cy 1): no gate
ALT = 256.5                                   # a float32 value


def _planted_gates(toa, alt32):
    """The hand-placed gates of a 7 x 3 scene: ``[(case, x, y, z_rel)]``.  The top of the kept heights is ``toa`` when it lies
    below the cell grid's ``z_hi``, ``z_hi`` otherwise; both exist among the scenes."""
    up, down = (lambda v: np.nextafter(F32(v), INF32)), (lambda v: np.nextafter(F32(v), -INF32))
    x_end, y_end = X0 + NCX * CELL, Y0 + NCY * CELL
    top = min(float(F32(toa)), Z_HI)
    g = []
    # interior boundaries in x, in cell row 0.  The boundary k = 4 is x = 0: the float32 below it is the negative denormal,
    # and x - x0 rounds to 4096 in float64 -- that gate belongs to cell 4, not 3
    for k in range(1, NCX):
        g.append(("x_boundary", X0 + k * CELL, Y0 + 300.0, 1000.0 + k))
        g.append(("x_below_boundary", down(X0 + k * CELL), Y0 + 300.0, 1000.0 + k))
    for k in range(1, NCY):                    # interior boundaries in y, in cell column 1
        g.append(("y_boundary", X0 + 1500.0, Y0 + k * CELL, 2000.0 + k))
        g.append(("y_below_boundary", X0 + 1500.0, down(Y0 + k * CELL), 2000.0 + k))
    g += [("x_at_origin", X0, Y0 + 10.0, 500.0), ("x_inside_origin", up(X0), Y0 + 10.0, 500.0),
          ("x_below_origin", down(X0), Y0 + 10.0, 500.0), ("x_at_end", x_end, Y0 + 10.0, 500.0),
          ("x_inside_end", down(x_end), Y0 + 10.0, 500.0),
          ("y_at_origin", X0 + 10.0, Y0, 500.0), ("y_inside_origin", X0 + 10.0, up(Y0), 500.0),
          ("y_below_origin", X0 + 10.0, down(Y0), 500.0), ("y_at_end", X0 + 10.0, y_end, 500.0),
          ("y_inside_end", X0 + 10.0, down(y_end), 500.0)]
    for x in (X0 + 700.0, X0 + 5 * CELL + 1.0):
        g += [("z_at_top", x, Y0 + 2100.0, top), ("z_above_top", x, Y0 + 2100.0, up(top)),
              ("z_at_lo", x, Y0 + 2100.0, Z_LO), ("z_below_lo", x, Y0 + 2100.0, down(Z_LO))]
    for coord in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            p = [X0 + 2000.0, Y0 + 2000.0, 700.0]
            p[coord] = bad
            g.append(("nonfinite", *p))
    g += [("duplicates", X0 + 4 * CELL + 77.25, Y0 + 1200.5, 3333.0)] * 5
    out = []
    for case, x, y, z_rel in g:
        gz = F32(z_rel) if not np.isfinite(z_rel) else _gz_for(z_rel, alt32)
        out.append((case, F32(x), F32(y), gz))
    return out


def _bulk(rng, n, cells, toa, alt32, avoid):
    """Random gates over a box somewhat larger than the cell grid (some fall outside), none in the cells ``avoid``."""
    x1, y1 = cells.x0 + cells.ncx * cells.cell, cells.y0 + cells.ncy * cells.cell
    pad = 0.15 * cells.cell
    gx = rng.uniform(cells.x0 - pad, x1 + pad, n).astype(np.float32)
    gy = rng.uniform(cells.y0 - pad, y1 + pad, n).astype(np.float32)
    top = min(float(toa), cells.z_hi)
    gz = (rng.uniform(cells.z_lo - 200.0, top + 200.0, n).astype(np.float32) + alt32).astype(np.float32)
    _, keep, cell = gate_cells(gx, gy, gz, alt32, toa, cells)
    for c in avoid:                            # move them one cell to the left (never column 0)
        gx = np.where(keep & (cell == c), gx - F32(cells.cell), gx).astype(np.float32)
    return gx, gy, gz


def _scene(name, gates, bulk, cells, alt32, toa, seed):
    """Planted gates and the bulk in one shuffled index order; ``planted[case]`` = the gate indices of a case."""
    cases = [c for c, *_ in gates]
    gx = np.concatenate([np.array([g[1] for g in gates], dtype=np.float32), bulk[0]])
    gy = np.concatenate([np.array([g[2] for g in gates], dtype=np.float32), bulk[1]])
    gz = np.concatenate([np.array([g[3] for g in gates], dtype=np.float32), bulk[2]])
    perm = np.random.default_rng(seed).permutation(gx.size)
    where = np.argsort(perm)                   # gate i of the unshuffled order sits at index where[i]
    planted = {}
    for i, c in enumerate(cases):
        planted.setdefault(c, []).append(int(where[i]))
    return SimpleNamespace(name=name, gx=gx[perm], gy=gy[perm], gz=gz[perm], alt=float(alt32), toa=float(toa), cells=cells,
                           planted={c: np.array(sorted(v)) for c, v in planted.items()}, n=int(gx.size))


@functools.lru_cache(maxsize=1)
def binning_scenes():
    """Hand-made cell grids for the single gate list.  7 x 3 cells of 1024 m with the origin at a multiple of the cell size:
    every planted boundary position is an exact float32 and the cell arithmetic is exact.  Gate counts 0, 1, 255, 256, 257
    and about 5000; ``toa`` below and above the cell grid's ``z_hi``; one scene with every gate dropped; a 1 x 1 grid; a grid
    with an arbitrary cell size for the random bulk.  The 7 x 3 scenes keep cell (3, 1) and the last cell empty."""
    alt32 = F32(ALT)
    cells = make_cells(X0, Y0, CELL, NCX, NCY, Z_LO, Z_HI)
    avoid = (EMPTY_MIDDLE, NCX * NCY - 1)
    scenes = []
    empty = tuple(np.zeros(0, dtype=np.float32) for _ in range(3))
    scenes.append(_scene("empty", [], empty, cells, alt32, 6000.0, 1))
    scenes.append(_scene("single", [("x_boundary", F32(X0 + 2 * CELL), F32(Y0 + 300.0), _gz_for(1000.0, alt32))], empty, cells,
                         alt32, 6000.0, 2))
    for k, (n, toa) in enumerate([(255, 6000.0), (256, 17000.0), (257, 6000.0), (5003, 17000.0), (4999, 6000.0)]):
        gates = _planted_gates(toa, alt32)
        rng = np.random.default_rng(100 + k)
        scenes.append(_scene(f"planted_{n}_toa{int(toa)}", gates, _bulk(rng, n - len(gates), cells, toa, alt32, avoid), cells,
                             alt32, toa, 10 + k))
    rng = np.random.default_rng(200)
    gx, gy, gz = _bulk(rng, 300, cells, 6000.0, alt32, ())
    gz = (gz + F32(7000.0)).astype(np.float32)           # every height above toa
    scenes.append(_scene("all_dropped", [], (gx, gy, gz), cells, alt32, 6000.0, 20))
    one = make_cells(-2048.0, -2048.0, 4096.0, 1, 1, Z_LO, Z_HI)
    scenes.append(_scene("one_cell", [], _bulk(np.random.default_rng(201), 257, one, 6000.0, alt32, ()), one, alt32, 6000.0, 21))
    odd = make_cells(-3000.3, -1411.1, 731.7, 9, 4, -300.0, 9000.0)
    scenes.append(_scene("odd_cells", [], _bulk(np.random.default_rng(202), 5000, odd, 17000.0, F32(0.0), ()), odd, F32(0.0),
                         17000.0, 22))
    return tuple(scenes)


def brute_force_bins(s):
    """``bin_gates_ref`` restated as a per-gate Python loop (for one small scene): ``(index order, cell_start)``."""
    c = s.cells
    per_cell = [[] for _ in range(c.ncx * c.ncy)]
    alt32, toa32 = F32(s.alt), F32(s.toa)
    for i in range(s.n):
        z_rel = F32(s.gz[i] - alt32)
        if not z_rel <= toa32 or not (c.z_lo <= float(z_rel) <= c.z_hi):
            continue
        fx, fy = (float(s.gx[i]) - c.x0) * c.inv_cx, (float(s.gy[i]) - c.y0) * c.inv_cy
        if not (np.isfinite(fx) and np.isfinite(fy)):
            continue
        tx, ty = int(np.floor(fx)), int(np.floor(fy))
        if 0 <= tx < c.ncx and 0 <= ty < c.ncy:
            per_cell[ty * c.ncx + tx].append(i)
    order = [i for cell in per_cell for i in cell]
    starts = np.concatenate([[0], np.cumsum([len(cell) for cell in per_cell])]).astype(np.int32)
    return np.array(order, dtype=np.int64), starts


# ---- per-level scenes ------------------------------------------------------------------------------------------------------
LEVEL_PARAMS = ((2500.0, 0.0), (250.0, 0.01746), (250.0, 0.3), (250.0, 0.45), (250.0, 0.499))     # (min_radius, beam_factor)
LEVEL_ALTS = (0.0, 437.25)
LEVEL_ZC = np.linspace(500.0, 8500.0, 9, dtype="float32")
N_LEVEL_EDGE = 60                             # planted gates per side of the reach bound


def _reach_f64(x, y, z, min_radius, bf):
    return max(min_radius, np.sqrt(x * x + y * y + z * z) * bf / (1.0 - bf))


@functools.lru_cache(maxsize=None)
def level_scene(min_radius, beam_factor, alt):
    """About 3000 random gates over the 7 x 3 cell grid plus gates planted at ``|z_rel - zc[k]| = R_g * (1 -+ 1e-4)`` -- just
    inside (must be listed under level k) and just outside (never) the reach bound, far from the free band of the inflation
    (1e-6 R_g + 1 mm) and from float32 rounding (below 1 mm at these heights).  ``R_g`` depends on the height looked for: the
    fixed point ``z = zc[k] -+ R_g(z) * (1 -+ 1e-4)`` is iterated in float64 (a contraction for bf < 0.5)."""
    alt32 = F32(alt)
    cells = make_cells(X0, Y0, CELL, NCX, NCY, -60000.0, 40000.0)
    rng = np.random.default_rng(int(1000 * beam_factor) + int(alt))
    gates = []
    for j in range(2 * N_LEVEL_EDGE):
        inside = j % 2 == 0
        k = int(rng.integers(len(LEVEL_ZC)))
        x, y = float(F32(rng.uniform(X0 + 50, X0 + NCX * CELL - 50))), float(F32(rng.uniform(Y0 + 50, Y0 + NCY * CELL - 50)))
        # above the level the fixed point runs away as bf / (1 - bf) approaches 1: those beams get gates below only
        side = -1.0 if (rng.random() < 0.5 or beam_factor > 0.31) else 1.0
        f = 1.0 - 1e-4 if inside else 1.0 + 1e-4
        z = float(LEVEL_ZC[k])
        for _ in range(200):
            z = float(LEVEL_ZC[k]) + side * _reach_f64(x, y, z, min_radius, beam_factor) * f
        gates.append(("inside" if inside else "outside", F32(x), F32(y), F32(z + float(alt32)), k))      # z_rel to 1 mm
    bulk = _bulk(rng, 3000, make_cells(X0, Y0, CELL, NCX, NCY, -1500.0, 12000.0), 17000.0, alt32, ())
    s = _scene(f"levels_bf{beam_factor}_alt{alt}", [g[:4] for g in gates], bulk, cells, alt32, 17000.0, 31)
    s.zc, s.min_radius, s.beam_factor = LEVEL_ZC, float(min_radius), float(beam_factor)
    s.planted_level = _planted_levels(s, gates)
    return s


def _planted_levels(s, gates):
    """index -> level of the planted gates: matched by their (unique) coordinates."""
    out = {}
    key = {(float(g[1]), float(g[2]), float(g[3])): (g[0], g[4]) for g in gates}
    assert len(key) == len(gates)
    for case in ("inside", "outside"):
        for i in s.planted[case]:
            c, k = key[(float(s.gx[i]), float(s.gy[i]), float(s.gz[i]))]
            assert c == case
            out[int(i)] = k
    return out


def level_scenes():
    return [level_scene(mr, bf, alt) for mr, bf in LEVEL_PARAMS for alt in LEVEL_ALTS]


# ---- gates exactly on the reach bound ----------------------------------------------------------------------------------------
ON_BOUND = dict(min_radius=250.0, beam_factor=0.45, num=9, den=11, step=20.0, nz=150)


@functools.lru_cache(maxsize=1)
def on_bound_scene():
    """Gates on the radar's vertical whose distance to a level is the reach bound itself.  With bf = 0.45 the bound is
    ``R_g = 9 |g| / 11``: a gate at height ``11 m`` lies exactly ``9 m`` from the levels ``2 m`` and ``20 m``.  Levels every
    20 m and float32-exact heights make every such |dz| exact, so only the float64 rounding of R_g itself decides on which
    side of it the pair falls -- the rounding the documented inflation of the lists exists for.  ``pairs``: the planted
    (level, gate index) pairs."""
    o = ON_BOUND
    zc = (np.arange(1, o["nz"] + 1) * o["step"]).astype(np.float32)
    gz, pairs = [], []
    for k, level in enumerate(zc.astype(np.float64)):
        for m in (level / (o["den"] - o["num"]), level / (o["den"] + o["num"])):       # the gate above / below the level
            z = o["den"] * m
            if 600.0 < z <= 16500.0 and float(F32(z)) == z and float(F32(o["num"] * m)) == o["num"] * m:
                pairs.append((k, len(gz)))
                gz.append(z)
    gz = np.array(gz, dtype=np.float32)
    zero = np.zeros(gz.size, dtype=np.float32)
    return SimpleNamespace(name="on_bound", gx=zero, gy=zero.copy(), gz=gz, alt=0.0, toa=17000.0, n=int(gz.size), zc=zc,
                           cells=make_cells(-2048.0, -2048.0, 4096.0, 1, 1, -100.0, 17000.0), min_radius=o["min_radius"],
                           beam_factor=o["beam_factor"], pairs=pairs, planted={})


# ---- the radar's vertical near the supported limit of beam_factor -----------------------------------------------------------
VERTICAL_BEAMS = (0.3, 0.45, 0.499)
VERTICAL_EPS = (1e-3, 1e-5, 1e-7)
VERTICAL_SHAPE = (7, 5, 5)
VERTICAL_LIMITS = ((1000.0, 10000.0), (-6000.0, 6000.0), (-6000.0, 6000.0))
VERTICAL_MIN_RADIUS = 250.0


@functools.lru_cache(maxsize=None)
def vertical_rim_scene(beam_factor, eps, n_background=1500, seed=3):
    """The case where the per-level reach bound is tight.  Odd ``ny`` / ``nx`` and symmetric xy limits put one voxel column
    on the radar's vertical; for every level k (``r_v = bf * zc[k] > min_radius``) one gate is planted at
    ``(0, 0, zc[k] - r_v (1 - eps))`` and one at ``(0, 0, zc[k] + r_v (1 - eps))``.  For the lower one
    ``R_g - |dz| = r_v eps / (1 - bf)``: the margin of the per-level bound goes to zero with eps.  Heights are float32: where
    rounding pushes a planted gate onto or beyond the rim (``dz^2 < r_v^2`` in float64 fails) it is stepped towards its voxel
    one float32 at a time, so every planted gate is a neighbour of its voxel.  A random background follows the planted gates.
    ``planted`` = ``[(voxel, gate index)]``."""
    nz, ny, nx = VERTICAL_SHAPE
    zc = np.linspace(*VERTICAL_LIMITS[0], nz, dtype="float32")
    gz, planted, margins = [], [], []
    for k in range(nz):
        zv = float(zc[k])
        r_v = max(VERTICAL_MIN_RADIUS, np.sqrt(0.0 + 0.0 + zv * zv) * beam_factor)
        assert r_v > VERTICAL_MIN_RADIUS
        for side in (-1.0, 1.0):
            z = F32(zv + side * r_v * (1.0 - eps))
            for _ in range(8):
                dz = float(z) - zv
                if dz * dz < r_v * r_v:
                    break
                z = np.nextafter(z, F32(zv))
            planted.append(((k * ny + ny // 2) * nx + nx // 2, len(gz)))
            margins.append(r_v - abs(float(z) - zv))
            gz.append(z)
    rng = np.random.default_rng(seed)
    n = len(gz)
    gx = np.concatenate([np.zeros(n, dtype=np.float32), rng.uniform(-8e3, 8e3, n_background).astype(np.float32)])
    gy = np.concatenate([np.zeros(n, dtype=np.float32), rng.uniform(-8e3, 8e3, n_background).astype(np.float32)])
    gz = np.concatenate([np.array(gz, dtype=np.float32), rng.uniform(0.0, 15e3, n_background).astype(np.float32)])
    return SimpleNamespace(shape=VERTICAL_SHAPE, limits=VERTICAL_LIMITS, min_radius=VERTICAL_MIN_RADIUS,
                           beam_factor=float(beam_factor), eps=float(eps), gx=gx, gy=gy, gz=gz, planted=planted,
                           margins=np.array(margins))


# ---- the sentinel, end to end ----------------------------------------------------------------------------------------------
SENTINEL_SHAPE = (3, 9, 70)
SENTINEL_LIMITS = ((500.0, 6000.0), (-3e3, 9e3), (-15e3, 15e3))
SENTINEL_ROI = dict(min_radius=1200.0, beam_factor=0.02)


@functools.lru_cache(maxsize=1)
def sentinel_scene():
    """4000 random gates around a ``(3, 9, 70)`` grid; field ``a`` carries the bit pattern of RG_EXCLUDED_BITS on about 1 % of
    its unmasked gates (``hot``), field ``a_ref`` the canonical quiet NaN in the same places and the same values elsewhere.  A
    gridding path that confuses such a value with the sentinel drops the gate and returns a number where the reference has
    NaN."""
    rng = np.random.default_rng(77)
    n = 4000
    gx = rng.uniform(-16e3, 16e3, n).astype(np.float32)
    gy = rng.uniform(-4e3, 10e3, n).astype(np.float32)
    gz = rng.uniform(0.0, 7e3, n).astype(np.float32)
    val = rng.normal(20.0, 10.0, n).astype(np.float32)
    mask = rng.random(n) < 0.15
    hot = np.zeros(n, dtype=bool)
    hot[rng.choice(np.nonzero(~mask)[0], 40, replace=False)] = True
    a, a_ref = val.copy(), val.copy()
    a.view(np.uint32)[hot] = EXCLUDED_BITS
    a_ref.view(np.uint32)[hot] = CANONICAL_NAN
    others = [rng.normal(0.0, 5.0, n).astype(np.float32) for _ in range(7)]
    other_masks = [rng.random(n) < 0.1 for _ in range(7)]
    return SimpleNamespace(shape=SENTINEL_SHAPE, limits=SENTINEL_LIMITS, gx=gx, gy=gy, gz=gz, a=a, a_ref=a_ref, mask=mask,
                           hot=hot, others=others, other_masks=other_masks, n=n, **SENTINEL_ROI)
