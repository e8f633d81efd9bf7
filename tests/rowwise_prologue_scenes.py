"""Hand-made CSR geometries for the chunk prologue and the pair test of the row-wise kernel over the packed records, and a
restatement of that pair test.  Plain NumPy: row pointers, gate indices and weights (in [0.02, 1], so that the 26-bit weight
code holds them); the tests push them through the library's own builder (``CompactCSR.build`` + ``ensure_packed``).

Grid (2, 5, 70): two segments of 35 rows per line, line groups of lines 0-3 and of line 4 alone (three wavefronts of the second
group's workgroups have no rows), eight chunks = (plane, line group, segment), 300 gates (every chunk keeps 14-byte records).
  chunk 0  (plane 0, lines 0-3, rows 0-34)    no pair: the first block of the dispatch order leaves early;
  chunk 1  (plane 0, lines 0-3, rows 35-69)   pairs in its fourth line only;
  chunks 2, 3  (plane 0, line 4)              pairs;
  chunks 4-7  (plane 1)                       variant "full": pairs everywhere, so the LAST block of the dispatch order -- chunk 6,
                                              which reads the final entries of rec_ptr and (chunk 7) dict_ptr -- has records;
                                              variant "empty": the whole plane has no pair, so that block leaves early.
A segment with pairs starts with the rows  0 1 0 1 1 0 2 3 4 5 200 0 5 4  pairs long: three one-pair rows in ONE record
with empty rows before, between and behind them, every length up to five, and a row that takes 67 records (23 steps of three at
one lane per row); the rest is drawn from 0-5, the last row is empty.  Row starts and row ends take every residue mod 3.
Field values include negative numbers, +-Inf, NaN and excluded gates.
"""
import numpy as np

LINES = 4                       # RG_COMPACT_LINES
ROTATION = 5                    # RG_COMPACT_ROTATION
SHAPE = (2, 5, 70)
N_GATES = 300
HEAD = (0, 1, 0, 1, 1, 0, 2, 3, 4, 5, 200, 0, 5, 4)
LENGTHS = (0, 1, 2, 3, 4, 5, 200)
VARIANTS = ("full", "empty")


def segments(shape=SHAPE):
    """``(line, sx, first row, rows, chunk)`` of every segment, line-major (lines counted through all planes)."""
    nz, ny, nx = shape
    nsx = (nx + 63) // 64
    nyg = (ny + LINES - 1) // LINES
    base, extra = divmod(nx, nsx)
    out = []
    for line in range(nz * ny):
        plane, y = divmod(line, ny)
        for sx in range(nsx):
            x0 = sx * base + min(sx, extra)
            out.append((line, sx, line * nx + x0, base + (1 if sx < extra else 0), (plane * nyg + y // LINES) * nsx + sx))
    return out


def dispatch_chunks(shape=SHAPE):
    """Chunk of block 0, 1, ... of the dispatch order (the rotation of ``block_chunk``)."""
    nz, ny, nx = shape
    nsx = (nx + 63) // 64
    nyg = (ny + LINES - 1) // LINES
    return [grp * nsx + (col + (grp * ROTATION) % nsx) % nsx for grp in range(nz * nyg) for col in range(nsx)]


def has_pairs(variant, line, sx, chunk):
    ny = SHAPE[1]
    plane, y = divmod(line, ny)
    if plane == 1:
        return variant == "full"
    if chunk == 0:
        return False
    if chunk == 1:
        return y == 3
    return True


def scene(variant):
    assert variant in VARIANTS
    rng = np.random.default_rng(5201 + VARIANTS.index(variant))
    nz, ny, nx = SHAPE
    lengths = np.zeros(nz * ny * nx, dtype=np.int64)
    for (line, sx, r0, nrows, chunk) in segments():
        if has_pairs(variant, line, sx, chunk):
            seg = rng.integers(0, 6, size=nrows)
            seg[:len(HEAD)] = HEAD
            seg[nrows - 1] = 0
            lengths[r0:r0 + nrows] = seg
    indptr = np.zeros(lengths.size + 1, dtype=np.int64)
    np.cumsum(lengths, out=indptr[1:])
    n_pairs = int(indptr[-1])
    gidx = rng.integers(0, N_GATES, size=n_pairs).astype(np.int32)
    wts = (0.02 + 0.98 * rng.random(n_pairs)).astype(np.float32)
    fields = [rng.normal(0, 20, N_GATES).astype(np.float32) for _ in range(8)]
    masks = [None] * 8
    masks[0] = rng.random(N_GATES) < 0.2
    masks[2] = rng.random(N_GATES) < 0.5
    masks[7] = rng.random(N_GATES) < 0.1
    free = np.nonzero(~masks[0])[0]
    fields[0][free[3]] = np.nan
    fields[0][free[40]] = np.inf
    fields[0][free[80]] = -np.inf
    fields[1][5] = -0.0
    fields[1][77] = np.inf
    fields[4][11] = -np.inf
    fields[7][200] = np.nan
    chunk_pairs = np.zeros(max(s[4] for s in segments()) + 1, dtype=np.int64)
    for (line, sx, r0, nrows, chunk) in segments():
        chunk_pairs[chunk] += int(indptr[r0 + nrows] - indptr[r0])
    return dict(shape=SHAPE, variant=variant, indptr=indptr, lengths=lengths, gidx=gidx, wts=wts, n_pairs=n_pairs,
                n_gates=N_GATES, fields=fields, masks=masks, chunk_pairs=chunk_pairs)


# ---- the pair test of the streaming loop ---------------------------------------------------------------------------------------
def step_state(qs, length, lanes, sub, steps, kpre=3, live=True):
    """``(lo0, len, q, q1)`` of lane ``sub`` of a row whose pairs are ``qs .. qs + length - 1`` of its segment, ``steps``
    batches of ``kpre`` records per lane after the row's first: what the kernel's ``setup`` and ``advance`` keep."""
    qe = qs + length if live else qs
    q0 = qs // 3
    q1 = (qe + 2) // 3 if qe > qs else q0
    q = q0 + sub
    lo0 = qs - 3 * q
    q += steps * kpre * lanes
    lo0 -= 3 * steps * kpre * lanes
    return lo0, qe - qs, q, q1


def pair_is_mine_kernel(lo0, length, lanes, k, i):
    """The kernel's test, against constants that depend on the slot ``k`` and the pair ``i`` alone: signed arithmetic."""
    return 3 * k * lanes + i < lo0 + length and (k > 0 or i == 2 or lo0 <= i)


def pair_is_mine_definition(qs, length, q, q1, lanes, k, i, live=True):
    """Pair ``i`` of batch slot ``k`` -- record ``q + k * lanes`` -- is the row's iff the slot holds one of the row's records
    and the pair's number in the segment lies in ``[qs, qs + length)``."""
    has = live and q + k * lanes < q1
    p = 3 * (q + k * lanes) + i
    return has and qs <= p < qs + length
