"""Scenes and plain-NumPy restatements shared by the record tests (test_gpu_dense_records.py) and the slab-seam tests
(test_gpu_slab_seams.py, test_slab_scenes.py).  Nothing here calls the code under test: the chunk layout, the dispatch
order, the record stream and the slab partition are restated from their descriptions (include/radargrid_hip.h,
csrc/rg_compact_layout.hpp, geometry_builder._build_compact_only's docstring), so that a test comparing the build with
them compares two independent derivations.

 1. layout: ``segment_starts`` / ``segments`` / ``chunk_of_rows`` / ``slot_table`` (both record orders) / ``slabs_for``;
 2. ``encode_records``: the packed record stream as bytes, the specification the pack kernel has to reproduce;
 3. ``make_slab_case``: a hand-made compact copy of a 5 x 7 x 130 grid whose planes are packed slab by slab;
 4. ``wide_scene``: a small radar scene that is three segments wide, with dense, wide and empty chunks and a level
    without pairs, and its oracle geometry (one brute-force build per process); ``wide_window_scene``: its first eight
    lines, where the dispatch order's rotation depends on a slab's first level.
"""
import functools

import numpy as np

from oracle import radar_grid_oracle as oracle

LINES = 4                    # grid lines per chunk                  (RG_COMPACT_LINES; the tests assert the equality)
ROTATION = 5                 # columns the dispatch order rotates per line group       (RG_COMPACT_ROTATION)
DENSE_MAX = 2048             # largest dictionary of a chunk with 14-byte records      (RG_DENSE_MAX_DICT)
ORDER_SEGMENT, ORDER_DISPATCH = 0, 1                                                 # RG_REC_ORDER_*
CODE_MAX = 0x3FFFFFF
W_BASE = 120 << 23           # Barnes and uniform weights span exponents 121 .. 127


# ---- 1. layout -----------------------------------------------------------------------------------------------------------
def layout(shape):
    """``(nsx, nyg, n_chunks)``: segments per line (at most 64 rows each), line groups per plane, chunks."""
    nz, ny, nx = shape
    nsx, nyg = (nx + 63) // 64, (ny + LINES - 1) // LINES
    return nsx, nyg, nz * nyg * nsx


def segment_starts(nx):
    """First row of every segment of a line, ``nx`` last: balanced, the first ``nx % nsx`` segments one row longer."""
    nsx = (nx + 63) // 64
    base, extra = divmod(nx, nsx)
    return [sx * base + min(sx, extra) for sx in range(nsx + 1)]


def segments(shape):
    """(line, sx, first row, rows, chunk) of every segment, line-major; lines count through all planes and the chunk of
    segment sx of line y of plane z is ``(z * nyg + y // LINES) * nsx + sx``."""
    nz, ny, nx = shape
    nsx, nyg, _ = layout(shape)
    starts = segment_starts(nx)
    out = []
    for line in range(nz * ny):
        plane, y = divmod(line, ny)
        for sx in range(nsx):
            out.append((line, sx, line * nx + starts[sx], starts[sx + 1] - starts[sx], (plane * nyg + y // LINES) * nsx + sx))
    return out


def chunk_of_rows(shape):
    """int64 ``[n_vox]``: the chunk of every row."""
    out = np.empty(int(np.prod(shape)), dtype=np.int64)
    for (_, _, r0, nrows, chunk) in segments(shape):
        out[r0:r0 + nrows] = chunk
    return out


def rotation_of_group(grp, nsx):
    """Columns by which the dispatch order rotates line group ``grp`` (counted through all planes of the WHOLE grid)."""
    return ((grp * ROTATION) & 0xFFFFFFFF) % nsx


def slot_table(shape, order):
    """``({(line, sx): slot}, n_slots)`` of a whole grid.  SEGMENT: the line-major segment number.  DISPATCH: workgroup b
    takes line group ``b // nsx`` and the column ``b % nsx`` rotated by that group's rotation; its wavefront w reads line
    ``4 * group's first line + w``, and the segment lies in slot ``4 b + w`` (slots of lines past a plane's end stay empty)."""
    nz, ny, nx = shape
    nsx, nyg, n_chunks = layout(shape)
    if order == ORDER_SEGMENT:
        return {(line, sx): line * nsx + sx for line in range(nz * ny) for sx in range(nsx)}, nz * ny * nsx
    table = {}
    for block in range(n_chunks):
        grp, col = divmod(block, nsx)
        sx = (col + rotation_of_group(grp, nsx)) % nsx
        plane, yg = divmod(grp, nyg)
        for w in range(LINES):
            if yg * LINES + w < ny:
                table[(plane * ny + yg * LINES + w, sx)] = block * LINES + w
    return table, n_chunks * LINES


def slabs_for(level_pairs, pairs_per_slab):
    """The slabs of whole levels the compact-only builder cuts: a slab takes levels while its pairs stay within
    ``pairs_per_slab``, and at least one.  ``[(first level, end level), ...]``."""
    out, iz0, nz = [], 0, len(level_pairs)
    while iz0 < nz:
        iz1, pairs = iz0 + 1, int(level_pairs[iz0])
        while iz1 < nz and pairs + int(level_pairs[iz1]) <= pairs_per_slab:
            pairs += int(level_pairs[iz1])
            iz1 += 1
        out.append((iz0, iz1))
        iz0 = iz1
    return out


def seam_level(level_pairs):
    """The first interior level i, with pairs in levels i and i + 1, at which ``pairs_per_slab = L[i] + L[i+1]`` makes some
    slab exactly full -- the ``<=`` of the rule at equality -- so that one pair less cuts the levels elsewhere.  ``None``
    when the level counts have no such level."""
    L = [int(v) for v in level_pairs]
    for i in range(1, len(L) - 2):
        cap = L[i] + L[i + 1]
        if L[i] and L[i + 1] and any(sum(L[a:b]) == cap for a, b in slabs_for(L, cap)) and slabs_for(L, cap) != slabs_for(L, cap - 1):
            return i
    return None


# ---- 2. the record stream ------------------------------------------------------------------------------------------------
def encode_records(case, shape, slot_of, n_slots, w_base=W_BASE):
    """The record stream as bytes + rec_ptr (16-byte units), restated from the layout's description.  ``case``: ``indptr``,
    ``pos`` (position of every pair in its chunk's dictionary), ``wts`` and ``sizes`` (dictionary entries per chunk);
    ``slot_of[(line, sx)]``: the segment's slot."""
    indptr, pos, sizes = case["indptr"], case["pos"], case["sizes"]
    code = case["wts"].view(np.uint32).astype(np.int64) - w_base
    assert code.min(initial=0) >= 0 and code.max(initial=0) <= CODE_MAX
    units = np.zeros(n_slots, dtype=np.int64)
    blobs = {}
    for (line, sx, r0, nrows, chunk) in segments(shape):
        p0, p1 = int(indptr[r0]), int(indptr[r0 + nrows])
        n = (p1 - p0 + 2) // 3
        c = np.zeros(3 * n, dtype=np.int64)
        p = np.zeros(3 * n, dtype=np.int64)
        c[:p1 - p0], p[:p1 - p0] = code[p0:p1], pos[p0:p1]
        c, p = c.reshape(n, 3), p.reshape(n, 3)
        if sizes[chunk] <= DENSE_MAX:                            # 14 bytes: seven halfwords, W2.hi moves in odd records
            assert p.max(initial=0) < 2048
            m1 = c[:, 0] | ((p[:, 1] & 0x3F) << 26)
            m2 = c[:, 1] | ((p[:, 2] & 0x3F) << 26)
            w2 = c[:, 2] | ((p[:, 2] >> 6) << 26)
            pw = p[:, 0] | ((p[:, 1] >> 6) << 11)
            lo, hi = (lambda x: x & 0xFFFF), (lambda x: x >> 16)
            even = np.stack([lo(w2), hi(w2), lo(m1), hi(m1), lo(m2), hi(m2), pw], axis=1)
            odd = np.stack([lo(w2), lo(m1), hi(m1), lo(m2), hi(m2), hi(w2), pw], axis=1)
            half = np.where((np.arange(n) % 2 == 1)[:, None], odd, even).astype("<u2")
            n_units = (14 * n + 15) // 16
            blob = np.zeros(16 * n_units, dtype=np.uint8)        # zero padding up to the next unit
            blob[:14 * n] = half.reshape(-1).view(np.uint8)
        else:                                                    # 16 bytes
            words = np.stack([c[:, 0] | ((p[:, 2] & 0x3F) << 26), c[:, 1] | (((p[:, 2] >> 6) & 0x3F) << 26),
                              c[:, 2] | ((p[:, 2] >> 12) << 26), p[:, 0] | (p[:, 1] << 16)], axis=1).astype("<u4")
            n_units = n
            blob = words.reshape(-1).view(np.uint8)
        units[slot_of[(line, sx)]] = n_units
        blobs[slot_of[(line, sx)]] = blob
    rec_ptr = np.zeros(n_slots + 1, dtype=np.int64)
    np.cumsum(units, out=rec_ptr[1:])
    stream = np.concatenate([blobs[s] for s in sorted(blobs)] + [np.zeros(0, dtype=np.uint8)])
    return stream, rec_ptr


# ---- 3. a hand-made compact copy to pack slab by slab ----------------------------------------------------------------------
SLAB_SHAPE = (5, 7, 130)     # 5 planes; 7 lines = a group of 4 and a ragged one of 3; 130 rows = segments of 44 / 43 / 43
SLAB_EMPTY_PLANE = 2
# dictionary entries per chunk, (plane, line group) per row of the table, one column per segment
SLAB_DICTS = [2048, 2049, 100, 3000, 2048, 2049,
              2500, 9, 2049, 2048, 65, 4000,
              0, 0, 0, 0, 0, 0,
              2049, 2048, 1, 2047, 700, 2048,
              2048, 2048, 2049, 5, 2049, 300]
SLAB_PARTITIONS = ([(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)], [(0, 2), (2, 3), (3, 5)], [(0, 5)])


@functools.lru_cache(maxsize=1)
def make_slab_case():
    """Row pointers, positions, dictionaries, gate indices, weights and fields of the hand-made geometry: every chunk's
    dictionary and every pair's position are chosen here, so the record stream is known without running any kernel.
    Plane 2 has no pairs (its slab is empty), one segment of plane 0 has none, every other segment starts with a row of
    at least 400 pairs, and most rows hold 0 .. 7."""
    shape = SLAB_SHAPE
    nz, ny, nx = shape
    nsx, nyg, n_chunks = layout(shape)
    rng = np.random.default_rng(77)
    sizes = np.array(SLAB_DICTS, dtype=np.int64)
    assert sizes.size == n_chunks
    n_vox = nz * ny * nx
    lengths = rng.choice([0, 0, 0, 1, 2, 3, 4, 5, 7], size=n_vox)
    segs = segments(shape)
    for (line, sx, r0, nrows, chunk) in segs:
        lengths[r0] = 400 + (line * nsx + sx) % 7
        lengths[r0 + 20] = 61
    lengths[SLAB_EMPTY_PLANE * ny * nx:(SLAB_EMPTY_PLANE + 1) * ny * nx] = 0
    line, sx, r0, nrows, _ = segs[1 * nsx + 1]                    # line 1, segment 1: no pairs
    lengths[r0:r0 + nrows] = 0
    indptr = np.zeros(n_vox + 1, dtype=np.int64)
    np.cumsum(lengths, out=indptr[1:])
    n_pairs = int(indptr[-1])
    chunk_of_pair = np.repeat(chunk_of_rows(shape), lengths)
    pos = (rng.integers(0, 1 << 30, size=n_pairs) % np.maximum(sizes, 1)[chunk_of_pair]).astype(np.int64)
    # every chunk with pairs uses its last dictionary entry: position 2047 in a dictionary of 2048, 2048 in one of 2049
    for c in np.nonzero(sizes)[0]:
        pos[np.nonzero(chunk_of_pair == c)[0][-1]] = sizes[c] - 1
    wts = (np.exp(-4.0 * rng.random(n_pairs)).astype(np.float32) + np.float32(1e-5))     # Barnes range: exponents 121 .. 127
    dict_ptr = np.zeros(n_chunks + 1, dtype=np.int64)
    np.cumsum(sizes, out=dict_ptr[1:])
    n_gates = int(dict_ptr[-1])
    dict_ = np.concatenate([dict_ptr[c] + rng.permutation(sizes[c]) for c in range(n_chunks)]).astype(np.int32)
    gidx = dict_[dict_ptr[chunk_of_pair] + pos]
    chunk_pairs = np.bincount(chunk_of_pair, minlength=n_chunks).astype(np.int64)
    fields = [rng.normal(10, 20, n_gates).astype(np.float32) for _ in range(8)]
    masks = [(rng.random(n_gates) < 0.2) if k % 2 == 0 else None for k in range(8)]
    fields[1][::7] = np.nan
    fields[0][2::19] = -0.0
    return dict(shape=shape, sizes=sizes, indptr=indptr, lengths=lengths, pos=pos, wts=wts, gidx=gidx, dict_ptr=dict_ptr,
                dict=dict_, n_gates=n_gates, n_pairs=n_pairs, chunk_pairs=chunk_pairs, chunk_of_pair=chunk_of_pair,
                fields=fields, masks=masks)


# ---- 4. the wide scene ---------------------------------------------------------------------------------------------------
WIDE_VOLUME = dict(n_elev=12, n_az=90, n_gates=60, seed=5, max_range_m=24e3)
WIDE_SHAPE = (6, 10, 150)
WIDE_LIMITS = ((0.0, 7500.0), (-3e3, 3e3), (-22e3, 22e3))
WIDE_KW = dict(min_radius=500.0)
WIDE_LEVEL_PAIRS = [47024, 4912, 1416, 460, 100, 0]
WIDE_WIDE_CHUNKS = [4224, 7023]              # dictionary sizes of the chunks with 16-byte records
WIDE_EMPTY_CHUNKS = 18
WIDE_LONGEST_ROW = 1073
# pairs_per_slab -> the slabs it has to give (slabs_for restates the rule; test_slab_scenes.py checks this table with it)
WIDE_SLABS = {1: [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6)], 6327: [(0, 1), (1, 2), (2, 6)],
              6328: [(0, 1), (1, 3), (3, 6)], 10 ** 12: [(0, 6)]}
WEIGHTINGS = ("barnes2", "cressman", "nearest")


@functools.lru_cache(maxsize=1)
def wide_volume():
    from radar_processor_amd import synthetic
    return synthetic.make_volume(**WIDE_VOLUME)


def _chunk_stats(shape, indptr, idx):
    """Pairs and distinct gates of every chunk of a CSR on ``shape``."""
    _, _, n_chunks = layout(shape)
    chunk_of_pair = np.repeat(chunk_of_rows(shape), np.diff(indptr))
    stride = int(idx.max(initial=0)) + 1
    distinct = np.unique(chunk_of_pair * stride + idx) // stride
    return np.bincount(chunk_of_pair, minlength=n_chunks), np.bincount(distinct, minlength=n_chunks)


@functools.lru_cache(maxsize=1)
def wide_scene():
    """The oracle geometry of the wide scene: ``indptr``, ``idx`` (rows sorted by gate index), per weighting the float64
    weights ``w64`` and their float32 roundings ``w32`` (one brute-force build; the other weightings are evaluated on the
    same neighbour sets), and per chunk its pairs and the number of distinct gates (``chunk_sizes``)."""
    vol = wide_volume()
    indptr, idx, _ = oracle.build_geometry(vol.gate_x, vol.gate_y, vol.gate_z, WIDE_SHAPE, WIDE_LIMITS, weighting="nearest",
                                           **WIDE_KW)
    w64 = {w: oracle.pair_weights_f64(indptr, idx, vol.gate_x, vol.gate_y, vol.gate_z, WIDE_SHAPE, WIDE_LIMITS, weighting=w,
                                      **WIDE_KW) for w in WEIGHTINGS}
    w32 = {w: w64[w].astype(np.float32) for w in WEIGHTINGS}
    chunk_pairs, chunk_sizes = _chunk_stats(WIDE_SHAPE, indptr, idx)
    return dict(vol=vol, shape=WIDE_SHAPE, indptr=indptr, idx=idx, w64=w64, w32=w32, chunk_pairs=chunk_pairs,
                chunk_sizes=chunk_sizes, level_pairs=np.diff(indptr[::WIDE_SHAPE[1] * WIDE_SHAPE[2]]))


# The wide scene has three line groups per level and three segments per line, so the rotation of the dispatch order, 5 columns
# per line group, comes to the same for every level: a slab's first level does not show in it.  Its first eight lines alone
# (``RoiSearch(window=WIDE_WINDOW)``: the same voxels, the same pairs) have two line groups, and the slab that starts at level
# p is rotated by p mod 3 columns more than a grid of its own would be.
WIDE_WINDOW = (0, 8, 0, 150)
WINDOW_SHAPE = (6, 8, 150)


@functools.lru_cache(maxsize=1)
def wide_window_scene():
    """The rows of ``wide_scene`` inside ``WIDE_WINDOW`` as a CSR of their own (NumPy row selection, no second build)."""
    w = wide_scene()
    nz, ny, nx = WIDE_SHAPE
    iy0, iy1, ix0, ix1 = WIDE_WINDOW
    rows = ((np.arange(nz)[:, None, None] * ny + np.arange(iy0, iy1)[None, :, None]) * nx
            + np.arange(ix0, ix1)[None, None, :]).ravel()
    lengths = np.diff(w["indptr"])[rows]
    indptr = np.zeros(rows.size + 1, dtype=np.int64)
    np.cumsum(lengths, out=indptr[1:])
    pairs = np.repeat(w["indptr"][rows] - indptr[:-1], lengths) + np.arange(int(indptr[-1]))
    idx = w["idx"][pairs]
    chunk_pairs, chunk_sizes = _chunk_stats(WINDOW_SHAPE, indptr, idx)
    return dict(vol=w["vol"], shape=WINDOW_SHAPE, indptr=indptr, idx=idx, w32={k: v[pairs] for k, v in w["w32"].items()},
                chunk_pairs=chunk_pairs, chunk_sizes=chunk_sizes,
                level_pairs=np.diff(indptr[::WINDOW_SHAPE[1] * WINDOW_SHAPE[2]]))
