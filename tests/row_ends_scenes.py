"""Hand-made CSR geometries for the row-end table of the row-wise kernel (``rg_csr_row_ends16``) and its early exit for
chunks without a record.  Plain NumPy: row pointers, gate indices and weights (in [0.02, 1], so that the 26-bit weight code
holds them); the tests push them through the library's own builder (``CompactCSR.build`` + ``ensure_packed``).

Scene A, grid (1, 6, 192): three segments of 64 rows per line, line groups of lines 0-3 and 4-5 (two wavefronts of the
second group's workgroups have no rows).  Chunk = (line group, segment):
  (0, 0)  four segments with spans 65534, 65535, 65536, 65537: both sides of the table's edge (RG_ROW_END16_MAX = 65534);
  (0, 1)  no pair at all: the early exit;
  (0, 2)  one pair in one row of one segment (span 1), the other three segments span 0;
  (1, 0)  a segment whose 70 000 pairs sit in ONE row (every row end is 0 or 70 000: the table cannot hold it), and a
          segment of short rows;
  (1, 1), (1, 2)  short rows: 0, 1, 2, 3, 4, 5 and 200 pairs, empty rows at the start, in the middle and at the end.
About a hundred distinct gates.

Scene B, grid (2, 8, 130): segments of 44 / 43 / 43 rows, 3000 gates.  The first chunk mentions 2600 gates (16-byte records)
and its first segment spans 66 000 pairs (row pointers); every other chunk stays below 2048 gates (14-byte records) and on
the 16-bit path, and the last chunk of the first plane has no pair.
"""
import numpy as np

LINES = 4                       # RG_COMPACT_LINES
ROW_END16_MAX = 65534           # RG_ROW_END16_MAX
SHAPE_A = (1, 6, 192)
SHAPE_B = (2, 8, 130)
EDGE_SPANS = (65534, 65535, 65536, 65537)
ONE_ROW_PAIRS = 70000
SHORT = (0, 1, 2, 3, 4, 5, 200)


def segments(shape):
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


def _spread(nrows, total):
    """Row lengths of a long segment: rows 0, nrows // 2 and nrows - 1 empty, rows 1-7 the SHORT lengths, the others share
    what is left of ``total``."""
    lengths = np.zeros(nrows, dtype=np.int64)
    lengths[1:8] = SHORT
    rest = [r for r in range(8, nrows - 1) if r != nrows // 2]
    left = total - int(lengths.sum())
    share, more = divmod(left, len(rest))
    for k, r in enumerate(rest):
        lengths[r] = share + (1 if k < more else 0)
    assert lengths.sum() == total
    return lengths


def _short_rows(rng, nrows):
    lengths = rng.choice(SHORT[:6], size=nrows)
    lengths[0] = lengths[nrows // 2] = lengths[nrows - 1] = 0
    lengths[3:10] = SHORT[::-1]
    return lengths


def _fields(rng, n_gates):
    """Eight fields; field 0 carries masked gates and an unmasked NaN, field 2 a mask of its own."""
    fields = [rng.normal(10, 20, n_gates).astype(np.float32) for _ in range(8)]
    masks = [None] * 8
    masks[0] = rng.random(n_gates) < 0.2
    masks[2] = rng.random(n_gates) < 0.5
    free = np.nonzero(~masks[0])[0]
    fields[0][free[len(free) // 2]] = np.nan
    fields[1][5] = -0.0
    return fields, masks


def _finish(shape, lengths, gidx_of, rng, n_gates):
    indptr = np.zeros(lengths.size + 1, dtype=np.int64)
    np.cumsum(lengths, out=indptr[1:])
    n_pairs = int(indptr[-1])
    gidx = np.empty(n_pairs, dtype=np.int32)
    for seg in segments(shape):
        p0, p1 = int(indptr[seg[2]]), int(indptr[seg[2] + seg[3]])
        gidx[p0:p1] = gidx_of(seg, p1 - p0)
    wts = (0.02 + 0.98 * rng.random(n_pairs)).astype(np.float32)
    fields, masks = _fields(rng, n_gates)
    spans = {(s[0], s[1]): int(indptr[s[2] + s[3]] - indptr[s[2]]) for s in segments(shape)}
    chunk_pairs = np.zeros(max(s[4] for s in segments(shape)) + 1, dtype=np.int64)
    for s in segments(shape):
        chunk_pairs[s[4]] += spans[(s[0], s[1])]
    return dict(shape=shape, indptr=indptr, lengths=lengths, gidx=gidx, wts=wts, n_pairs=n_pairs, n_gates=n_gates,
                fields=fields, masks=masks, spans=spans, chunk_pairs=chunk_pairs)


def scene_a():
    rng = np.random.default_rng(1601)
    nz, ny, nx = SHAPE_A
    lengths = np.zeros(nz * ny * nx, dtype=np.int64)
    for (line, sx, r0, nrows, chunk) in segments(SHAPE_A):
        if sx == 0 and line < 4:
            lengths[r0:r0 + nrows] = _spread(nrows, EDGE_SPANS[line])
        elif (line, sx) == (2, 2):
            lengths[r0 + 20] = 1
        elif (line, sx) == (4, 0):
            lengths[r0 + 30] = ONE_ROW_PAIRS
        elif line >= 4 and (line, sx) != (5, 1):
            lengths[r0:r0 + nrows] = _short_rows(rng, nrows)
    n_gates = 128
    return _finish(SHAPE_A, lengths, lambda seg, n: rng.integers(0, 100, size=n), rng, n_gates)


def scene_b():
    rng = np.random.default_rng(1602)
    nz, ny, nx = SHAPE_B
    nsx = 3
    empty_chunk = 1 * nsx + 2                    # plane 0, second line group, last segment
    lengths = np.zeros(nz * ny * nx, dtype=np.int64)
    for (line, sx, r0, nrows, chunk) in segments(SHAPE_B):
        if (line, sx) == (0, 0):
            lengths[r0:r0 + nrows] = _spread(nrows, 66000)
        elif chunk != empty_chunk:
            lengths[r0:r0 + nrows] = rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 9, 11], size=nrows)

    def gidx_of(seg, n):
        if (seg[0], seg[1]) == (0, 0):
            return np.arange(n) % 2600            # every gate below 2600: a wide chunk
        return 2600 + (seg[4] * 30 + rng.integers(0, 300, size=n)) % 400
    return _finish(SHAPE_B, lengths, gidx_of, rng, 3000)


SCENES = {"A": scene_a, "B": scene_b}
