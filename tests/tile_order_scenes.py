"""Hand-made CSR geometries for the tile kernels' order of float32 additions (``csrc/rg_row_phase.hpp``), checked bit for bit
against ``oracle.csr_apply_tile_order``.  Plain NumPy: every row length is chosen here, so a test decides where a row sits
relative to a tile boundary and how many rows share a tile.

A scene is a grid shape plus one *recipe* per segment (a line of nx rows holds ceil(nx / 64) balanced segments): the lengths
of the segment's rows from its first row on, the rest of its rows empty.  A row may carry a *kind* (special gates, below) and
a *class* (a label the tests look rows up by).

Scenes
  seams<T>, T in TILES   grid (1, 42, 64): one segment of 64 rows per line, 42 segments (not a multiple of the 4 wavefronts
                         of a workgroup).  Rows of T-1, T, T+1, 2T, 2T+1 and 3T+5 pairs starting at segment offsets 0, 1 and
                         T-1; rows that end / start exactly at a tile boundary (the latter long
                         enough to cross the next boundary of every other tile); a row longer than two tiles between short
                         rows; one tile-sized segment per active-row span of SPANS (every lane split L = 64 ... 1, at a power
                         of two and just above it); two rows 40 empty rows apart (span 42: L = 1) and the SAME pairs in
                         adjacent rows of another segment (L = 32); the special rows; a segment without a pair; a segment
                         with empty rows at both ends; last a single row of T+1 pairs, so that the last pair of the whole
                         array is the first pair of a tile -- it refers to gate n_gates - 1.
  line1                  grid (2, 3, 1): six segments of one row (0, 5, 130, 1, 600 and 2 pairs).
  line63, line65         grids (1, 5, 63) and (1, 5, 65): segments of 63 rows, and of 33 / 32.
  line130                grid (1, 6, 130): six lines of three segments (44 / 43 / 43 rows), which the kernels rotate per line.
  wide130                line130's rows over 4096 gates: three of its chunks (4 lines x one segment) refer to more than 2048
                         distinct gates, so their packed records are the 16-byte ones (14 bytes everywhere else), and to more
                         than the LDS window of an 8-field pass holds (the per-pair path next to windowed chunks).
  empty                  grid (1, 3, 70) without a single pair.

Gates (N_GATES = 512; wide130: 4096, the additional ones ordinary).  480-487 are excluded in fields 1 and 5 and in no other field; 488-493 carry, in every field and
excluded in none, NaN, +Inf, -Inf, -0.0, a denormal and the bits of RG_EXCLUDED_BITS (an unmasked value: ``rg_pack_fields_f32``
stores it as the canonical quiet NaN, it is data).  Only rows with a kind refer to 480-493.
Fields: normal(0, 1) * 2^uniform(-12, 12), mixed signs; fields 1, 3, 5, 7 have masks of their own, fields 0, 2, 4, 6 none.
Weights: exp(-4 u) + 1e-5, the Barnes range (exponents 121 .. 127: codable for the packed records).
"""
import numpy as np

from oracle import radar_grid_oracle as oracle

TILES = (128, 192, 256, 320, 384, 512)
SPANS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)          # active-row spans: L = 64 32 16 16 8 8 4 4 2 2 1 1
LANES_OF_SPAN = {s: 1 << ((64 // s).bit_length() - 1) for s in SPANS}
LENGTH_CLASSES = ("T-1", "T", "T+1", "2T", "2T+1", "3T+5")
SEAM_CLASSES = tuple("len " + n for n in LENGTH_CLASSES) + ("ends at a boundary", "starts at a boundary", "long between short")
EXCLUDED_BITS = 0x7FD1CE5D                                  # RG_EXCLUDED_BITS
N_GATES = 512
N_FIELDS = 8
WIDE_GATES = 4096                                           # gates of "wide130": chunks of more than 2048 distinct gates
MASKED_GATES = np.arange(480, 488)
G_NAN, G_PINF, G_MINF, G_NEGZERO, G_DENORM, G_EXCL = 488, 489, 490, 491, 492, 493
ORDINARY = np.r_[0:480, 494:512]
MASKED_FIELDS = (1, 5)                                      # the fields that exclude MASKED_GATES
MASK_RATE = {1: 0.2, 3: 0.5, 5: 0.1, 7: 0.3}
# the largest field count whose table accepts the tile: its restatement holds that of every smaller count (same order per field)
WIDEST = {128: 8, 192: 3, 256: 4, 320: 4, 384: 4, 512: 2}


def tiles_for(nf):
    """The tiles ``rg_row_phase.hpp``'s table accepts for ``nf`` fields, its default included."""
    return oracle.TILE_ORDER_ACCEPTED[nf]


def segments(shape):
    """``(line, sx, first row, rows)`` of every segment, line-major (lines counted through all planes)."""
    nz, ny, nx = shape
    nsx = (nx + 63) // 64
    base, extra = divmod(nx, nsx)
    return [(line, sx, line * nx + sx * base + min(sx, extra), base + (1 if sx < extra else 0))
            for line in range(nz * ny) for sx in range(nsx)]


def R(n, kind=None, cls=None):
    return (int(n), kind, cls)


def _shorts(rng, k, hi=10):
    return [R(v) for v in rng.integers(1, hi, size=k)]


def _special_rows(T):
    return [R(0)] * 3 + [R(9, "nan"), R(5, "pinf"), R(12, "minf"), R(7, "pminf"), R(3, "negzero"), R(1, "denorm"), R(6, "excl"),
                         R(10, "masked"), R(1, "masked"), R(2), R(1), R(T + 30, "nan"), R(2, "excl"), R(0), R(1)]


def _build(name, shape, recipes, seed, twins=(), tile=None, n_gates=N_GATES):
    """Row pointers, gates, weights, fields and masks of a scene.  ``twins``: pairs (b, a) of segment numbers -- segment b gets
    the gates and weights of segment a, pair by pair."""
    rng = np.random.default_rng(seed)
    segs = segments(shape)
    assert len(recipes) <= len(segs), (name, len(recipes), len(segs))
    recipes = list(recipes) + [[]] * (len(segs) - len(recipes))
    n_rows = int(np.prod(shape))
    lengths = np.zeros(n_rows, dtype=np.int64)
    kinds, classes = {}, {}
    for (line, sx, r0, nrows), rows in zip(segs, recipes):
        assert len(rows) <= nrows, (name, line, sx, len(rows), nrows)
        for k, (n, kind, cls) in enumerate(rows):
            lengths[r0 + k] = n
            if kind is not None:
                kinds[r0 + k] = kind
            if cls is not None:
                classes.setdefault(cls, []).append(r0 + k)
    indptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(lengths, out=indptr[1:])
    n_pairs = int(indptr[-1])
    gidx = rng.choice(np.r_[ORDINARY, N_GATES:n_gates], size=n_pairs).astype(np.int32)
    wts = (np.exp(-4.0 * rng.random(n_pairs)).astype(np.float32) + np.float32(1e-5))
    for r, kind in kinds.items():
        p0, p1 = int(indptr[r]), int(indptr[r + 1])
        mid = (p0 + p1) // 2
        if kind == "nan":
            gidx[mid] = G_NAN
        elif kind == "pinf":
            gidx[mid] = G_PINF
        elif kind == "minf":
            gidx[mid] = G_MINF
        elif kind == "pminf":
            gidx[p0], gidx[p1 - 1] = G_PINF, G_MINF
        elif kind == "excl":
            gidx[mid] = G_EXCL
        elif kind == "negzero":
            gidx[p0:p1] = G_NEGZERO
        elif kind == "denorm":
            gidx[p0:p1] = G_DENORM
        elif kind == "masked":
            gidx[p0:p1] = rng.choice(MASKED_GATES, size=p1 - p0)
        else:
            raise ValueError(kind)
    for b, a in twins:
        a0, a1 = (int(indptr[segs[a][2]]), int(indptr[segs[a][2] + segs[a][3]]))
        b0, b1 = (int(indptr[segs[b][2]]), int(indptr[segs[b][2] + segs[b][3]]))
        assert a1 - a0 == b1 - b0
        gidx[b0:b1], wts[b0:b1] = gidx[a0:a1], wts[a0:a1]
    if n_pairs:
        gidx[-1] = n_gates - 1
    fields, masks = [], []
    for f in range(N_FIELDS):
        v = (rng.normal(0.0, 1.0, n_gates) * np.exp2(rng.uniform(-12.0, 12.0, n_gates))).astype(np.float32)
        v[G_NAN], v[G_PINF], v[G_MINF], v[G_NEGZERO], v[G_DENORM] = np.nan, np.inf, -np.inf, -0.0, 1e-40
        v.view(np.uint32)[G_EXCL] = EXCLUDED_BITS
        fields.append(v)
        if f in MASK_RATE:
            m = rng.random(n_gates) < MASK_RATE[f]
            m[480:494] = False
            m[MASKED_GATES] = f in MASKED_FIELDS
            masks.append(m)
        else:
            masks.append(None)
    return dict(name=name, shape=shape, indptr=indptr, lengths=lengths, gidx=gidx, wts=wts, n_pairs=n_pairs, n_gates=n_gates,
                fields=fields, masks=masks, kinds=kinds, classes={k: np.asarray(v) for k, v in classes.items()}, tile=tile)


# Seeds of the seam scenes' gates, weights and fields, chosen so that the scenes discriminate (test_tile_order_scenes.py: with
# values spread over 24 binades two orders of a sum agree in all bits for about one row in three; a seed under which a whole
# class of rows did so was passed over)
SEAM_SEEDS = {128: 8328, 192: 7392, 256: 8456, 320: 7520, 384: 7584, 512: 8712}


def seam_scene(T):
    rng = np.random.default_rng(7100 + T)
    segs = []
    lens = dict(zip(LENGTH_CLASSES, (T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 5)))
    for start in (0, 1, T - 1):
        for cname, n in lens.items():
            segs.append(([R(start)] if start else []) + [R(n, cls="len " + cname)] + _shorts(rng, 3))
    ends, starts = "ends at a boundary", "starts at a boundary"
    segs.append([R(T // 2 - 5), R(T - (T // 2 - 5), cls=ends), R(T // 2 + 70, cls=starts)] + _shorts(rng, 2))
    segs.append([R(T + 10), R(T - 10, cls=ends), R(T // 2 + 90, cls=starts)] + _shorts(rng, 2))
    segs.append([R(7), R(T - 7, cls=ends), R(T // 2 + 33, cls=starts)] + _shorts(rng, 4))
    for before, after in ((9, 5), (3, 17), (20, 2)):
        segs.append(_shorts(rng, before, hi=6) + [R(2 * T + 40, cls="long between short")] + _shorts(rng, after))
    for s in SPANS:                                          # s non-empty rows from the segment's first row on, one tile
        if s == 64:
            row_lens = rng.integers(1, 3, size=64)
        else:
            row_lens = rng.integers(max(1, T // s // 2), T // s + 1, size=s)
        assert row_lens.sum() <= T
        segs.append([R(n, cls=f"span {s}") for n in row_lens])
    apart = len(segs)
    segs.append([R(61, cls="gap apart")] + [R(0)] * 40 + [R(53, cls="gap apart")])
    segs.append([R(61, cls="gap adjacent"), R(53, cls="gap adjacent")])
    segs.append(_special_rows(T))
    segs.append([])                                          # a segment without a pair
    segs.append([R(0)] * 5 + _shorts(rng, 20))               # empty rows at both ends
    segs.append([R(T + 1, cls="last row")])
    assert len(segs) == 42
    return _build(f"seams{T}", (1, len(segs), 64), segs, SEAM_SEEDS[T], twins=((apart + 1, apart),), tile=T)


def _random_rows(rng, nrows):
    n = rng.choice([0, 0, 0, 1, 2, 3, 5, 8, 13, 21], size=nrows)
    long_rows = rng.random(nrows) < 0.04
    n[long_rows] = rng.integers(100, 700, size=int(long_rows.sum()))
    return [R(v) for v in n]


def line_scene(nx, n_gates=N_GATES, name=None):
    rng = np.random.default_rng(7300 + nx)
    if nx == 1:
        return _build("line1", (2, 3, 1), [[R(0)], [R(5)], [R(130)], [R(1)], [R(600)], [R(2)]], 7301)
    shape = (1, 6, 130) if nx == 130 else (1, 5, nx)
    recipes = [_random_rows(rng, nrows) for (_, _, _, nrows) in segments(shape)]
    recipes[1] = []                                                                  # a segment without a pair
    recipes[2] = [R(0)] * 4 + _random_rows(rng, segments(shape)[2][3] - 9)           # empty rows at both ends
    recipes[3] = _special_rows(128)
    recipes[-1] = recipes[-1][:-1] + [R(385)]                                        # the last row of the grid crosses tiles
    return _build(name or f"line{nx}", shape, recipes, 7400 + nx, n_gates=n_gates)


def empty_scene():
    return _build("empty", (1, 3, 70), [], 7500)


SCENES = {**{f"seams{T}": (lambda T=T: seam_scene(T)) for T in TILES},
          **{f"line{nx}": (lambda nx=nx: line_scene(nx)) for nx in (1, 63, 65, 130)},
          "wide130": lambda: line_scene(130, n_gates=WIDE_GATES, name="wide130"),
          "empty": empty_scene}
SEAM_SCENES = tuple(f"seams{T}" for T in TILES)
DATA_SCENES = tuple(n for n in SCENES if n != "empty")


# ---- helpers shared by the CPU and the GPU test --------------------------------------------------------------------------------
class Restatements:
    """``oracle.csr_apply_tile_order`` per (scene, field count, tile, fill), computed once.  The order is the same for every
    field count that accepts a tile (each field by the same rule with its own mask: ``test_tile_order_scenes`` checks the
    restatement for it), so one run with the WIDEST count per (scene, tile) serves all narrower ones; it is made with a
    finite fill, whose rows are exactly the rows without a live pair, and other fills are written over those."""

    FILL = np.float32(-9999.0)

    def __init__(self):
        self._scenes, self._wide, self.used = {}, {}, set()

    def scene(self, name):
        if name not in self._scenes:
            self._scenes[name] = SCENES[name]()
        return self._scenes[name]

    def filled(self, name, nf):
        """bool [nf, rows]: the rows without a pair that the field does not exclude (all weights are positive)."""
        c = self.scene(name)
        n_rows = c["lengths"].size
        row_of = np.repeat(np.arange(n_rows), c["lengths"])
        out = np.empty((nf, n_rows), dtype=bool)
        for f in range(nf):
            live = np.ones(c["n_pairs"], dtype=bool) if c["masks"][f] is None else ~c["masks"][f][c["gidx"]]
            out[f] = np.bincount(row_of[live], minlength=n_rows) == 0
        return out

    def wide(self, name, tile):
        if (name, tile) not in self._wide:
            c = self.scene(name)
            nf = WIDEST[tile]
            got = oracle.csr_apply_tile_order(c["indptr"], c["gidx"], c["wts"], c["fields"][:nf], c["masks"][:nf], c["shape"],
                                              tile=tile, fill_value=self.FILL, used=self.used).reshape(nf, -1)
            assert np.array_equal(got == self.FILL, self.filled(name, nf)), (name, tile)
            self._wide[(name, tile)] = got
        return self._wide[(name, tile)]

    def get(self, name, nf, tile=0, fill=np.nan):
        """float32 [nf, rows] for ``tile`` (0 = the default of the field count)."""
        tile = tile or oracle.TILE_ORDER_DEFAULT[nf]
        if tile not in tiles_for(nf):
            raise ValueError((nf, tile))
        return np.where(self.filled(name, nf), np.float32(fill), self.wide(name, tile)[:nf]).astype(np.float32)


def sequential_mean(c, f):
    """The masked weighted mean of field ``f`` with plain left-to-right float32 sums per row (NaN where nothing is live)."""
    out = np.full(c["lengths"].size, np.nan, dtype=np.float32)
    live = np.ones(c["n_pairs"], dtype=bool) if c["masks"][f] is None else ~c["masks"][f][c["gidx"]]
    w = np.where(live, c["wts"], np.float32(0)).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        p = np.where(live, c["wts"] * c["fields"][f][c["gidx"]], np.float32(0)).astype(np.float32)
        for r in np.nonzero(c["lengths"])[0]:
            p0, p1 = int(c["indptr"][r]), int(c["indptr"][r + 1])
            sp = np.add.accumulate(p[p0:p1], dtype=np.float32)[-1]
            sw = np.add.accumulate(w[p0:p1], dtype=np.float32)[-1]
            if sw > 0:
                out[r] = np.float32(np.float64(sp) / np.float64(sw))
    return out


def same_bits(a, b):
    """Per element: both NaN, or the same float32 bits."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return (np.isnan(a) & np.isnan(b)) | (a.view(np.int32) == b.view(np.int32))
