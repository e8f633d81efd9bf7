"""How a geometry is stored, which CSR kernel a pass runs through, with which LDS window, and how many fields it fuses:
every threshold and every decision of the host side, as plain functions of numbers and booleans.

Host code only -- nothing here imports ``torch``, loads the library or touches a device, so the whole policy can be read
and tested on a CPU.  The callers (``gridding``, ``plane_products``, ``grid_geometry``, ``geometry_builder``) look the
facts up -- pair counts, free memory, what the device CSR holds -- and ask here.  Anything expensive or with a side effect
(building the compact copy, packing the records, asking the driver for free memory) is handed in as a callable and called
exactly when the decision needs it.

The three kernels of a CSR pass (ms per pass on config 2 / the bench grid, MI355X):

                                 1 field        2 fields       3 fields       4 fields       8 fields
    rg_csr_apply_f32             1.9 / 13.1     2.1 / 14.7     2.3 / 16.5     3.0 / 20.5     7.3 / 49.8
    compact, tile kernel         1.11 / 8.4     1.69 / 11.6    2.2 / 14.6     3.3 / 19.5     9.6 / 65
    compact, row-wise kernel     1.02 / 7.9     1.13 / 8.7     1.29 / 10.1    1.47 / 10.3    3.9 / 14.4

The row-wise kernel reads the packed records (weights codable in 26 bits: Barnes, nearest) and has no tile in LDS, so it
wins at every window it can hold.  The tile kernel (weights not codable) wins while its window stays <= 24 KiB next to its
tiles and loses beyond; a compact-only geometry has no choice.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional, Tuple

from ._native import RG_MAX_FIELDS

GIB = 1 << 30

# ---- thresholds, each defined once ------------------------------------------------------------------------------------------
LARGE_GEOMETRY_PAIRS = 50_000_000   # below this a pass takes well under a millisecond either way: no compact copy by default
                                    # (use_compact), and layout="auto" keeps the reference's arrays (choose_layout)
TILE_WINDOW_MAX_BYTES = 24576       # tile kernel: LDS window beyond which the standard kernel is the faster one (table above)
MAX_FALLBACK_SHARE = 0.02           # share of pairs allowed on the per-pair path before the standard kernel is preferred
PIPELINE_TILES = (128, 192, 256, 320, 384, 512)   # pairs per pipeline step the tile kernels accept (0 = their default)
COLUMNS_MIN_WORKGROUPS = 8192       # column kernel: cut columns into level pieces until the launch has about this many workgroups
COLUMNS_MAX_FIELDS = 4              # the column / planes modes of the row-wise kernel (the products epilogue) take 1-4 fields
COLUMNS_FUSE_MIN_FIELDS = 5         # fused=None: fields per pass from which the products epilogue would pay in TIME -- more
                                    # than COLUMNS_MAX_FIELDS, so never by default (see run_fused)
LDS_BUDGET_BYTES = 32768            # window budget of a pass: 5 workgroups per CU
LDS_BUDGET_ROWWISE_BYTES = 49152    # row-wise kernel, 3-8 fields: entries carry mask bytes and have no tile next to them
STANDARD_VOLUMES_PER_PASS = 4       # rg_csr_apply_f32, bench grid: 20.7 ms for four field-volumes, 55.1 for eight

KERNEL_STANDARD = "rg_csr_apply_f32"                    # the reference's arrays
KERNEL_TILE = "rg_csr_compact_apply_f32"                # compact copy, plain positions and weights
KERNEL_ROWWISE = "rg_csr_compact_apply_packed_f32"      # compact copy, packed records (row-wise kernel; tile 384: tile kernel)


# ---- window arithmetic -------------------------------------------------------------------------------------------------------
def entry_bytes(n_fields: int, rowwise: bool = False) -> int:
    """Bytes of one LDS window entry of the compact kernels.  Tile kernels: the packed slots of a gate (1, 2, 4 or 8
    floats; a 3-field entry without its padding slot).  Row-wise kernel (``rowwise``): one field the value and a 0/1
    factor, two fields the two values, three and more the values (v' = value or +0) plus one mask byte per field -- 16,
    20 and 40 bytes for 3, 4 and 5-8 fields (``csrc/rg_compact_layout.hpp``: rowwise_entry_words)."""
    if rowwise and n_fields >= 3:
        return 16 if n_fields == 3 else 20 if n_fields == 4 else 40
    if n_fields > 4:
        return 32
    return 4 * (2 if n_fields <= 2 else 3 if n_fields == 3 else 4)


def window_for(window_cap: int, n_fields: int, rowwise: bool = False, lds_budget_bytes: Optional[int] = None) -> int:
    """LDS window (entries) for a pass of ``n_fields`` fields: the geometry's 99.9 % window ``window_cap`` if its entries
    fit ``lds_budget_bytes`` (default ``LDS_BUDGET_BYTES``; ``LDS_BUDGET_ROWWISE_BYTES`` for the row-wise kernel's 3-8 field
    entries), else the largest multiple of 64 that does."""
    if lds_budget_bytes is None:
        lds_budget_bytes = LDS_BUDGET_ROWWISE_BYTES if (rowwise and n_fields >= 3) else LDS_BUDGET_BYTES
    room = max(0, lds_budget_bytes // entry_bytes(n_fields, rowwise)) // 64 * 64
    return int(min(window_cap, room))


# ---- memory: free device memory a step wants before it allocates (bytes per pair + a margin, each written once, here) -------
def compact_copy_fits(n_pairs: int, free_bytes: int) -> bool:
    """Room for the compact copy of a CSR (16-bit positions + dictionaries): more than 3.2 bytes per pair + 8 GiB."""
    return free_bytes > 3.2 * n_pairs + 8 * GIB


def packed_records_fit(n_pairs: int, free_bytes: int) -> bool:
    """Room for the packed records next to the compact copy (5.4 bytes per pair): 5.6 bytes per pair + 6 GiB."""
    return free_bytes >= 5.6 * n_pairs + 6 * GIB


def settle_copies_fit(record_bytes: int, tries: int, grid_bytes: int, free_bytes: int) -> bool:
    """Room for ``tries - 1`` further copies of the record array and the probe's output grids + 8 GiB
    (``CsrGridder.settle_records``)."""
    return free_bytes >= (tries - 1) * record_bytes + grid_bytes + 8 * GIB


def choose_layout(n_pairs: int, free_bytes: int, weighting_is_codable: bool) -> str:
    """``compute_grid_geometry(layout="auto")``.  Large geometries whose weights fit the 26-bit code (Barnes, uniform) are
    built in the packed layout ALONE: row pointers + dictionaries + 16-byte records, 5.4 bytes per pair -- it is what every
    gridding pass of 1-8 fields reads anyway, the reference's index and weight arrays are rebuilt from it on demand, bit
    for bit, and a process touches 47 GB instead of 115 GB for the bench geometry (first-touch allocation is what a build's
    wall time consists of).  Geometries below ``LARGE_GEOMETRY_PAIRS`` grid in well under a millisecond either way and keep
    the reference's arrays; non-codable weights (Cressman) keep them too while they and their compact copy fit, and fall to
    the compact layout otherwise."""
    if n_pairs >= LARGE_GEOMETRY_PAIRS and weighting_is_codable:
        return "packed"
    return "csr" if 10.4 * n_pairs + 10 * GIB <= free_bytes else "compact"      # the reference's arrays + their compact copy


def weight_code_base(lo_exp: int, hi_exp: int) -> Optional[int]:
    """Base exponent of the records' 26-bit weight code for weights whose float32 exponent fields (bits >> 23; a sign bit
    shows as an exponent >= 256) span ``lo_exp .. hi_exp``, or ``None`` when they are not codable: the base is a multiple of
    8 (the kernels OR it back in), all weights are positive normal numbers and span at most 8 binades above it."""
    base = lo_exp & ~7
    if lo_exp <= 0 or hi_exp - base > 7 or hi_exp >= 255:
        return None
    return base


# ---- the kernel of a pass ----------------------------------------------------------------------------------------------------
class CopyFacts(NamedTuple):
    """What the decisions below ask of a compact copy (``grid_geometry.CompactCSR``); ``copy_of`` callables yield one."""
    window_cap: int                                 # LDS window (entries) that covers 99.9 % of the pairs
    fallback_fraction: Callable[[int], float]       # share of the pairs in chunks with more distinct gates than a window
    ensure_packed: Callable[[], bool]               # build the packed records if they can be built: do they exist?
    compact: object = None                          # the copy itself, for the caller


class PassChoice(NamedTuple):
    """What :func:`choose_pass` decided."""
    kernel: str             # KERNEL_STANDARD / KERNEL_TILE / KERNEL_ROWWISE
    window: int             # LDS window (entries); 0 without the compact copy
    use_compact: bool       # the pass runs through the compact copy
    packed_stream: bool     # ... and streams its packed records
    copy: object            # what ``copy_of`` yielded when ``use_compact``, else None


def choose_pass(n_fields: int, n_pairs: int, has_gate_indices: bool, has_weights: bool, compact: bool, packed: bool,
                copy_of: Callable[[], object]) -> PassChoice:
    """The kernel of a pass of ``n_fields`` fields over a device CSR of ``n_pairs`` pairs that holds (or not) the reference's
    ``gate_indices`` / ``weights`` arrays, for a caller who asks for the compact copy (``compact``) and its records
    (``packed``).  ``copy_of()`` yields the compact copy or ``None``; of the copy only ``window_cap``,
    ``fallback_fraction(window)`` and ``ensure_packed()`` (build the records if they can be built: do they exist?) are used.

    * The copy is looked up only for a caller who wants it or a geometry that has nothing else, and never for an empty
      geometry.
    * A copy next to the reference's arrays is turned down when the TILE kernel's window for this field count leaves more
      than ``MAX_FALLBACK_SHARE`` of the pairs to the per-pair path (dense scans next to many fields: the standard kernel is
      faster).  The tile kernel's window is the yardstick whichever kernel the pass ends up on.
    * Passes of 1-8 fields stream the packed records (positions + weights, 5.33 bytes per pair) when the caller wants them,
      or the geometry holds no weights besides them, and they exist; the window is then the row-wise kernel's.
    * Without the records, a copy next to the reference's arrays is turned down when its window exceeds
      ``TILE_WINDOW_MAX_BYTES``."""
    copy = copy_of() if ((compact or not has_gate_indices) and n_pairs) else None
    window, stream = 0, False
    if copy is not None:
        window = window_for(copy.window_cap, n_fields)
        if has_gate_indices and copy.fallback_fraction(window) > MAX_FALLBACK_SHARE:
            copy, window = None, 0
    if copy is not None:
        stream = bool((packed or not has_weights) and copy.ensure_packed())
        if stream:
            window = window_for(copy.window_cap, n_fields, rowwise=True)
        elif has_gate_indices and window * entry_bytes(n_fields) > TILE_WINDOW_MAX_BYTES:
            copy, window = None, 0
    kernel = KERNEL_STANDARD if copy is None else KERNEL_ROWWISE if stream else KERNEL_TILE
    return PassChoice(kernel, window, copy is not None, stream, copy)


def tile_override(tile: int, packed_stream: bool, has_compact: bool, has_weights: bool) -> Tuple[str, int]:
    """``(entry point, its tile argument)`` for the diagnostic ``tile`` of ``CsrGridder``: 0 = default; 128...512 the
    pipeline tile of the tile kernels (non-default values change the order of the float32 adds); 384 also selects the tile
    kernel over the packed records; 2000 + h the lane split of the row-wise kernel.  A gridder that streams records leaves
    them for another pipeline tile only where the plain arrays exist."""
    if has_compact and packed_stream and (tile in (0, 384) or tile >= 2000 or not has_weights):
        return KERNEL_ROWWISE, tile if (tile == 384 or tile >= 2000) else 0
    return (KERNEL_TILE if has_compact else KERNEL_STANDARD), tile if tile in PIPELINE_TILES else 0


def has_columns_kernel(use_compact: bool, packed_stream: bool, n_fields: int) -> bool:
    """The column and planes modes of the row-wise kernel read the packed records: 1-4 fields, codable weights."""
    return bool(use_compact and packed_stream and n_fields <= COLUMNS_MAX_FIELDS)


def column_pieces(nz: int, n_columns: int) -> int:
    """Level pieces per column of chunks such that a column-mode launch has about ``COLUMNS_MIN_WORKGROUPS`` workgroups."""
    return max(1, min(nz, -(-COLUMNS_MIN_WORKGROUPS // max(n_columns, 1))))


# ---- pass sizes --------------------------------------------------------------------------------------------------------------
def use_compact(cached_copy_state: Optional[bool], n_pairs: int, free_bytes: Callable[[], int]) -> bool:
    """Policy of ``grid_fields_device`` / ``apply_geometry``: a geometry large enough to matter grids through the compact
    copy of its CSR from its FIRST pass on, provided the memory is there -- the one-time conversion costs about as much as
    building the geometry did (15 ms per 1e9 pairs for the copy, as much again for the packed records), and deciding by
    size alone means that every pass of a geometry runs the same kernel and returns the same bits.  ``cached_copy_state``:
    ``None`` while no copy was tried for this device CSR; otherwise whether the try gave one, which then decides (once
    built the copy is always used).  ``free_bytes()`` is asked only for a large geometry without a cached answer."""
    if cached_copy_state is not None:
        return bool(cached_copy_state)
    if n_pairs < LARGE_GEOMETRY_PAIRS:
        return False
    return compact_copy_fits(n_pairs, free_bytes())


def records_copy(n_pairs: int, has_weights: bool, use_compact: bool, copy_of: Callable[[], object]) -> Tuple[bool, object]:
    """Will the passes ``grid_fields_device`` cuts stream the packed records?  ``(yes or no, the compact copy that holds
    them)``.  A geometry without weights has nothing else (its copy is looked up, not asked); otherwise yes iff the compact
    copy is wanted, the geometry has pairs, and the records exist or can be built.  The fall-back share plays no part."""
    if not has_weights:
        return True, copy_of()
    if use_compact and n_pairs:
        copy = copy_of()
        if copy is not None and copy.ensure_packed():
            return True, copy
    return False, None


def fields_per_pass(n_pairs: int, has_weights: bool, use_compact: bool, copy_of: Callable[[], object]) -> int:
    """Fields one CSR pass should fuse.  Through the packed records (the row-wise kernel, 1-8 fields): 8 where the geometry's
    LDS window holds 40-byte entries within ``LDS_BUDGET_BYTES`` (bench grid: one pass of eight 15.5 ms against two of four
    2 x 10.5), 4 where it does not (config 2's 1792-entry window: one pass of eight 3.4-3.9 ms against 2 x 1.4); 8
    (``RG_MAX_FIELDS``) through the other kernels."""
    _, copy = records_copy(n_pairs, has_weights, use_compact, copy_of)
    if copy is not None:
        return 8 if copy.window_cap * entry_bytes(8, rowwise=True) <= LDS_BUDGET_BYTES else 4
    return RG_MAX_FIELDS


def volumes_per_pass_cap(n_pairs: int, has_weights: bool, use_compact: bool, copy_of: Callable[[], object]) -> int:
    """Field-volumes of a batch one pass should fuse (``batch.VolumeBatch``): what the packed records take (8 or 4, see
    :func:`fields_per_pass`), ``STANDARD_VOLUMES_PER_PASS`` otherwise.  Measured on the bench grid (ms per fused pass):
    row-wise kernel over the packed records 7.9 / 8.7 / 10.1 / 10.5 / 15.5 for 1 / 2 / 3 / 4 / 8 field-volumes (1.9 ms each
    at eight, where the geometry's LDS window admits eight), ``rg_csr_apply_f32`` 13.1 / 14.9 / 18.8 / 20.7 and 55.1 for
    eight; the CSR-free gridder keeps gaining up to 8 because it shares the whole neighbour search."""
    streams, _ = records_copy(n_pairs, has_weights, use_compact, copy_of)
    if streams:
        return fields_per_pass(n_pairs, has_weights, use_compact, copy_of)
    return min(STANDARD_VOLUMES_PER_PASS, RG_MAX_FIELDS)


def run_fused(columns_kernel: bool, profile_products: bool, n_fields: int, fused: Optional[bool]) -> bool:
    """Does a group of ``grid_products_device`` take its planes out of the gridding kernel's epilogue?  Only where the
    gridder has the column mode (:func:`has_columns_kernel`) and no profile product needs the stored grid; then on request
    (``fused=True``).  Measured (profiles/r04_columns_variants_*.json, r04_nf4_lds_rowsums.json): walking columns costs what the store it saves costs -- 8.2 vs 8.1 ms for one field, 10.7 vs
    10.5 for three, 11.4 vs 11.2 for four on the bench grid -- so the epilogue is the MEMORY-saving choice (no F x 640 MB of
    grid) and ``fused=None`` grids, then reduces: ``COLUMNS_FUSE_MIN_FIELDS`` is more than the column mode takes."""
    return bool(columns_kernel and not profile_products
                and (n_fields >= COLUMNS_FUSE_MIN_FIELDS if fused is None else bool(fused)))
