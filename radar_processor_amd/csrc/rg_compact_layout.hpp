// Layout of the compact CSR copy shared by the K1c kernels (rg_csr_compact.hip: the tile kernels, and the description of the
// layout at its head; rg_csr_rowwise.hpp: the row-wise kernel, with its grid mode in rg_csr_rowwise.hip and its column and planes
// modes in rg_csr_columns.hip; rg_csr_pack.hip, rg_csr_compact_build.hip: what writes the copy): chunk grid, block -> chunk rotation, segments,
// buffer resources, record codings, per-field-count tuning of the row-wise kernel, and the argument checks the entry points
// over the packed records share.  Everything here has internal linkage on purpose (each translation unit gets its own copy;
// nothing is exported) except the launcher declared at the end.
#pragma once

#include <type_traits>

#include "rg_common.hpp"
#include "rg_row_phase.hpp"

// 16-byte buffer load by intrinsic name (this compiler's __builtin_amdgcn_raw_buffer_load_b128 returns the first dword
// in every element, see rg_csr_apply.hip); namespace scope: a name bound to an intrinsic must not have internal linkage.
using rg_u32x4 = unsigned __attribute__((ext_vector_type(4)));
__device__ rg_u32x4 rg_buffer_load_v4u32(__amdgpu_buffer_rsrc_t, int voffset, int soffset, int aux)
    __asm("llvm.amdgcn.raw.ptr.buffer.load.v4i32");

// v_mul_legacy_f32 by intrinsic name (this clang has no __builtin_amdgcn_fmul_legacy): 0 * x = +0 for EVERY x, NaN and
// infinity included; any other product is the IEEE one.
__device__ float rg_fmul_legacy(float, float) __asm("llvm.amdgcn.fmul.legacy");

// Types that cross translation units (the launcher at the end of this file) live in a NAMED namespace: a function with a parameter of an anonymous-namespace type has no linkage.
namespace rgl {

// Where a chunk's wavefronts find their rows: the grid as planes x lines x rows (nz x ny x nx for a radar grid).
// Chunk arithmetic is 32-bit on purpose: every wavefront decodes its chunk number with two divisions, and a 64-bit
// division costs this ISA a few hundred instructions (measured: 7 % of the single-field kernel).
struct ChunkGrid {
  long line_len;            // rows per line (nx)
  long lines_per_plane;     // lines per plane (ny)
  long n_planes;            // planes (nz)
  unsigned nsx;             // segments per line = ceil(line_len / 64)
  unsigned nyg;             // line groups per plane = ceil(lines_per_plane / H)
  unsigned rot_step;        // columns the block -> chunk map rotates per line group (speed only)
  unsigned seg_base;        // a line's nsx segments are balanced: the first seg_extra hold seg_base + 1 rows, the
  unsigned seg_extra;       // others seg_base (<= 64 either way) -- rg_csr_apply_f32 cuts its lines the same way
  unsigned grp0;            // line groups in front of this grid when it is a slab of whole planes of a larger one
                            // (rg_csr_compact_pack's plane0 * nyg; 0 for the apply kernels): the rotation counts them
};

// ---- column mode of the row-wise kernel (rg_csr_compact_apply_columns_f32) ----
struct RowwiseColumns {
  const int32_t* order = nullptr;   // optional: workgroup -> piece * n_cols + column (heaviest first)
  float* planes = nullptr;          // [F][n_keep][n_xy] or null
  float* col_val = nullptr;         // [pieces][F][n_xy] (pieces == 1: the caller's plane) or null
  int32_t* col_arg = nullptr;       // same shape, or null
  long n_xy = 0;
  unsigned n_cols = 0;              // line groups per plane x segments per line
  int pieces = 1, keep_lo = 0, n_keep = 0, col_lo = 0, col_hi = 0;
};

// ---- planes mode: the column mode with the wider epilogue (rg_csr_compact_apply_planes_f32) ----
// A separate type, so that the column mode's kernel argument -- and its code -- stays what it was.
struct RowwisePlanes : RowwiseColumns {
  float* col_min = nullptr;                             // [pieces][F][n_xy] (pieces == 1: the caller's plane) or null
  float* col_mean = nullptr;                            // [F][n_xy] or null (pieces == 1 only)
  const int32_t* sel[RG_MAX_SEL_PLANES] = {};           // n_sel planes [n_xy]: lo | hi << 16, or RG_PPI_SEL_NONE
  float* samples = nullptr;                             // [F][n_sel][2][n_xy]
  int n_sel = 0;
};

// ---- the arguments the three entry points over the packed records share: rg_csr_compact_apply_packed_f32, _columns_f32 and
// _planes_f32 (their 17 leading ones, and what each passes on to its launcher) -- checked by check_stream_args ----
struct StreamArgs {
  const void* indptr;
  bool is_i64;
  const void* records;
  const int64_t* rec_ptr;
  int rec_order;
  unsigned w_base;
  const int64_t* dict_ptr;
  const int32_t* dict;
  long n_vox, n_pairs, line_len, lines_per_plane;
  const float* packed;
  int n_fields, stride;
  long n_gates;
  float fill;
  float* out;
  int window_cap;
  int lanes_hint;          // 0 = from the segment's mean row length, a power of two up to 64, or 70 + records per lane and row
  hipStream_t stream;
  // where the entry points differ
  int max_fields;          // 8 for rg_csr_compact_apply_packed_f32 (whose tile kernel refuses 5-8 itself); 4 for the other two
  bool need_out;           // the grid is all rg_csr_compact_apply_packed_f32 produces; the other two may store planes only
  bool need_packed;        // column / planes modes: packed fields present and 16-byte aligned even without a pair
  // the _ex variants of the three entry points
  const uint16_t* row_end16 = nullptr;   // rg_csr_row_ends16's table of the same grid, or null: every segment reads indptr
};

}  // namespace rgl

namespace {

using rgl::ChunkGrid;
using rgl::StreamArgs;
using rgl::RowwiseColumns;
using rgl::RowwisePlanes;
using rg::f32x2;
using rg::f32x4;
using rsrc_t = __amdgpu_buffer_rsrc_t;
constexpr int kRsrcRaw32 = 0x00020000;   // gfx9 buffer resource word 3: DATA_FORMAT = 32, untyped access

__device__ __forceinline__ rsrc_t make_rsrc(const void* base, long bytes) {   // `base` and `bytes` wave-uniform
  const unsigned nb = bytes >= 0xFFFFFFFFL ? 0xFFFFFFFFu : bytes <= 0 ? 0u : (unsigned)bytes;
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)nb, kRsrcRaw32);
}

constexpr int kH = RG_COMPACT_LINES;   // grid lines (= wavefronts) per chunk

// Workgroups are dealt to the 8 XCDs round-robin by blockIdx.  With nsx segments per line a multiple of 8, chunk column
// sx would always land on XCD sx % 8 and each XCD would own one x-slab of the grid for the whole launch; rotating the
// columns by rot_step per line group makes every XCD see every column.  The chunk a workgroup takes is a bijection of
// blockIdx; with RG_REC_ORDER_DISPATCH the records are STORED in this order (see rg_csr_compact_pack), so the map is part
// of the layout: grid_geometry.CompactCSR.slot_of_segments restates it.
__device__ __forceinline__ unsigned block_chunk(const ChunkGrid& g, unsigned bid) {
  const unsigned grp = bid / g.nsx;
  const unsigned col = bid - grp * g.nsx;
  const unsigned rot = col + ((grp + g.grp0) * g.rot_step) % g.nsx;
  return grp * g.nsx + (rot >= g.nsx ? rot - g.nsx : rot);
}

__host__ __device__ inline long chunk_count(const ChunkGrid& g) { return g.n_planes * (long)g.nyg * (long)g.nsx; }

struct Segment {
  long r0;      // first row
  long seg;     // segment number, line-major: (plane * lines_per_plane + line) * nsx + sx
  int nrows;    // 0 for a wavefront past the last line of the plane
};

__device__ __forceinline__ Segment chunk_segment(const ChunkGrid& g, unsigned chunk, int w) {   // chunk < 2^31
  const unsigned grp = chunk / g.nsx;         // line group, counted through all planes
  const unsigned sx = chunk - grp * g.nsx;
  const unsigned plane = grp / g.nyg;
  const unsigned yg = grp - plane * g.nyg;
  const long y = (long)yg * kH + w;
  Segment s;
  if (y >= g.lines_per_plane) {
    s.r0 = 0;
    s.seg = 0;
    s.nrows = 0;
    return s;
  }
  s.seg = ((long)plane * g.lines_per_plane + y) * g.nsx + sx;
  const unsigned x0 = sx * g.seg_base + (sx < g.seg_extra ? sx : g.seg_extra);
  s.r0 = ((long)plane * g.lines_per_plane + y) * g.line_len + (long)x0;
  s.nrows = (int)(g.seg_base + (sx < g.seg_extra ? 1u : 0u));
  return s;
}

using rg::stride_for;

// ---- the packed records: two codings, chosen per CHUNK by the size of its dictionary ---------------------------------------
// A record is three consecutive pairs of a segment: three 26-bit weight codes (float32 bits - w_base) and three positions.
//   WIDE  (16 bytes, 16-bit positions), every chunk with more than RG_DENSE_MAX_DICT dictionary entries (split chunks too):
//     [w0:26 | p2 bits 0-5] [w1:26 | p2 bits 6-11] [w2:26 | p2 bits 12-15] [p0:16 | p1:16]; record q at byte 16 * q.
//   DENSE (14 bytes, 11-bit positions), every chunk with at most RG_DENSE_MAX_DICT = 2048 entries.  Three words and a half:
//     M1 = w0:26 | p1 bits 0-5     M2 = w1:26 | p2 bits 0-5     W2 = w2:26 | p2 bits 6-10 | 0     P = p0:11 | p1 bits 6-10  (16 bits)
//     stored as seven little-endian halfwords from byte 14 * q of the segment's (16-byte aligned) records:
//       q even:  W2.lo W2.hi M1.lo M1.hi M2.lo M2.hi P           q odd:  W2.lo M1.lo M1.hi M2.lo M2.hi W2.hi P
//     A reader loads the ALIGNED 16 bytes d0..d3 at (14 * q) & ~3 -- the record starts at byte 0 of the load when q is even
//     and at byte 2 when it is odd -- and finds M1 = d1 and M2 = d2 either way.  With sh = 16 * (q & 1):
//       W2 = ({d3, d0} >> sh) & 0xFFFFFFFF  (one v_alignbit_b32: d0 itself, or d0.hi | d3.lo << 16)      P = (d3 >> sh) & 0xFFFF
//     so the parity costs one funnel shift and two bit-field offsets, no select.
// rec_ptr counts 16-byte UNITS in both codings: a segment of n records starts on a 16-byte boundary and takes n units (wide)
// or ceil(14 * n / 16) units (dense); the last record's load never leaves them (n odd leaves >= 2 bytes of padding).
constexpr int kDenseMaxDict = RG_DENSE_MAX_DICT;
__host__ __device__ inline bool rec_is_dense(long nd_all) { return nd_all <= kDenseMaxDict; }
__host__ __device__ inline long rec_units(long n_rec, bool dense) { return dense ? (14 * n_rec + 15) >> 4 : n_rec; }

struct RecFields {      // a decoded record: weight codes still carry the position bits above bit 25
  unsigned wc[3];
  unsigned pos[3];
};

// `ld`: the 16 bytes loaded for the record; `par` (dense only): any word whose bit 0 is the parity of the record's number in
// its segment.  Shift amounts reach the instructions unmasked where the hardware takes them modulo 32 anyway.
template <bool DENSE>
__device__ __forceinline__ RecFields rec_decode(const rg_u32x4& ld, unsigned par) {
  RecFields r;
  if constexpr (DENSE) {
    const unsigned sh = par << 4;                                   // v_alignbit_b32 / v_bfe_u32 read bits 0-4 of it: 0 or 16
    const unsigned w2 = __builtin_amdgcn_alignbit(ld.w, ld.x, sh);
    r.wc[0] = ld.y;
    r.wc[1] = ld.z;
    r.wc[2] = w2;
    r.pos[0] = __builtin_amdgcn_ubfe(ld.w, sh, 11u);
    const unsigned p1h = __builtin_amdgcn_ubfe(ld.w, sh + 11u, 5u);
    r.pos[1] = __builtin_amdgcn_alignbit(p1h, ld.y, 26);           // ld.y >> 26 | p1h << 6
    r.pos[2] = __builtin_amdgcn_alignbit(w2 >> 26, ld.z, 26);      // ld.z >> 26 | (w2 >> 26) << 6
  } else {
    r.wc[0] = ld.x;
    r.wc[1] = ld.y;
    r.wc[2] = ld.z;
    r.pos[0] = ld.w & 0xFFFFu;
    r.pos[1] = ld.w >> 16;
    unsigned p2b = ld.y >> 26, p2c = ld.z >> 26;
    asm volatile("" : "+v"(p2b), "+v"(p2c));     // keep the shifts apart: each OR then folds into a v_lshl_or_b32
    r.pos[2] = (p2c << 12) | ((p2b << 6) | (ld.x >> 26));
  }
  return r;
}

// The seven halfwords of a dense record in storage order (the pack kernel; the inverse of rec_decode<true>).
__device__ __forceinline__ void rec_encode_dense(const unsigned (&code)[3], const unsigned (&pos)[3], bool odd, unsigned short (&h)[7]) {
  const unsigned m1 = (code[0] & 0x3FFFFFFu) | ((pos[1] & 0x3Fu) << 26);
  const unsigned m2 = (code[1] & 0x3FFFFFFu) | ((pos[2] & 0x3Fu) << 26);
  const unsigned w2 = (code[2] & 0x3FFFFFFu) | (((pos[2] >> 6) & 0x1Fu) << 26);
  const unsigned short p = (unsigned short)((pos[0] & 0x7FFu) | (((pos[1] >> 6) & 0x1Fu) << 11));
  const unsigned short m1l = (unsigned short)m1, m1h = (unsigned short)(m1 >> 16), m2l = (unsigned short)m2,
                       m2h = (unsigned short)(m2 >> 16), w2h = (unsigned short)(w2 >> 16);
  h[0] = (unsigned short)w2;
  h[1] = odd ? m1l : w2h;
  h[2] = odd ? m1h : m1l;
  h[3] = odd ? m2l : m1h;
  h[4] = odd ? m2h : m2l;
  h[5] = odd ? w2h : m2h;
  h[6] = p;
}

bool make_chunk_grid(int64_t n_rows, int64_t line_len, int64_t lines_per_plane, ChunkGrid* cg) {
  if (line_len <= 0) line_len = n_rows > 0 ? n_rows : 1;
  if (n_rows % line_len != 0) return false;
  const long n_lines = n_rows / line_len;
  if (lines_per_plane <= 0) lines_per_plane = n_lines > 0 ? n_lines : 1;
  if (n_lines % lines_per_plane != 0) return false;
  cg->line_len = line_len;
  cg->lines_per_plane = lines_per_plane;
  cg->n_planes = n_lines / lines_per_plane;
  const long nsx = (line_len + 63) / 64, nyg = (lines_per_plane + kH - 1) / kH;
  if (nsx > 0x7FFFFFFFL || nyg > 0x7FFFFFFFL) return false;
  cg->nsx = (unsigned)nsx;
  cg->nyg = (unsigned)nyg;
  cg->seg_base = (unsigned)(line_len / nsx);
  cg->seg_extra = (unsigned)(line_len % nsx);
  // measured on the bench grid (32 columns), ms per launch: 0 -> 14.2 (every XCD keeps its columns), 8 -> 10.5,
  // 1 -> 9.35, 2 -> 9.27, 3 -> 9.24, 5 -> 9.23, 7 -> 9.21, 9 -> 9.22, 11 -> 9.31, 17 -> 9.22
  cg->rot_step = RG_COMPACT_ROTATION;
  cg->grp0 = 0;
  return true;
}

// Validates what `fn`, one of the three entry points over the packed records, shares with the other two, and builds the chunk
// grid (left alone when n_vox == 0: nothing to launch).  RG_OK, or the status to return with the error text set.
inline int check_stream_args(const char* fn, const StreamArgs& a, ChunkGrid* cg) {
  RG_REQUIRE(a.rec_order == RG_REC_ORDER_SEGMENT || a.rec_order == RG_REC_ORDER_DISPATCH, RG_EINVAL,
             "%s: rec_order=%d is neither RG_REC_ORDER_SEGMENT nor RG_REC_ORDER_DISPATCH", fn, a.rec_order);
  RG_REQUIRE(a.n_fields >= 1 && a.n_fields <= a.max_fields, RG_EUNSUPPORTED, "%s: n_fields=%d not in 1..%d", fn, a.n_fields,
             a.max_fields);
  RG_REQUIRE(a.stride == stride_for(a.n_fields), RG_EINVAL, "%s: stride=%d, expected %d for %d fields", fn, a.stride,
             stride_for(a.n_fields), a.n_fields);
  RG_REQUIRE(a.indptr && a.dict_ptr && a.rec_ptr && (a.out || !a.need_out), RG_EINVAL, "%s: null indptr/dict_ptr/rec_ptr%s", fn,
             a.need_out ? "/out" : "");
  RG_REQUIRE(a.n_vox >= 0 && a.n_pairs >= 0, RG_EINVAL, "%s: negative size", fn);
  RG_REQUIRE(a.n_pairs == 0 || (a.records && a.dict && a.packed && a.n_gates > 0), RG_EINVAL,
             "%s: pairs present but records/dict/packed/n_gates missing", fn);
  RG_REQUIRE(!a.need_packed || (a.packed && a.n_gates > 0), RG_EINVAL, "%s: packed fields missing", fn);
  RG_REQUIRE(a.n_gates <= 0x7FFFFFFFL, RG_EUNSUPPORTED, "%s: n_gates exceeds int32 gate indices", fn);
  RG_REQUIRE(a.n_vox <= 0x3FFFFFFFFFL, RG_EUNSUPPORTED, "%s: n_vox too large for one launch", fn);
  RG_REQUIRE(a.window_cap >= 0 && a.window_cap <= RG_COMPACT_MAX_WINDOW, RG_EINVAL, "%s: window_cap %d outside 0..%d", fn,
             a.window_cap, RG_COMPACT_MAX_WINDOW);
  RG_REQUIRE(rg::aligned16(a.records), RG_EALIGN, "%s: records must be 16-byte aligned", fn);
  RG_REQUIRE(!a.need_packed || rg::aligned16(a.packed), RG_EALIGN, "%s: packed must be 16-byte aligned", fn);
  RG_REQUIRE((a.w_base & 0x3FFFFFFu) == 0, RG_EINVAL,
             "%s: w_base=0x%08x must have its low 26 bits clear (exponent a multiple of 8)", fn, a.w_base);
  RG_REQUIRE(a.lanes_hint == 0 || (a.lanes_hint >= 1 && a.lanes_hint <= 64 && (a.lanes_hint & (a.lanes_hint - 1)) == 0) ||
                 (a.lanes_hint > 70 && a.lanes_hint <= 99), RG_EINVAL,
             "%s: the lane split must be 0, a power of two up to 64, or 71..99", fn);
  if (a.n_vox == 0) return RG_OK;
  RG_REQUIRE(make_chunk_grid(a.n_vox, a.line_len, a.lines_per_plane, cg), RG_EINVAL,
             "%s: n_vox=%ld is not planes x lines_per_plane=%ld x line_len=%ld", fn, a.n_vox, a.lines_per_plane, a.line_len);
  RG_REQUIRE(chunk_count(*cg) <= 0x7FFFFFFFL, RG_EUNSUPPORTED, "%s: too many chunks for one launch", fn);
  return RG_OK;
}

// ---- per-field-count configuration of the row-wise kernels (see rg_csr_rowwise.hpp for what the knobs mean) ----
template <int NF> struct RowwiseConfig;
template <> struct RowwiseConfig<1> { static constexpr int kpre = 3, target = 4; static constexpr bool regs = false; };
template <> struct RowwiseConfig<2> { static constexpr int kpre = 3, target = 4; static constexpr bool regs = false; };
template <> struct RowwiseConfig<3> { static constexpr int kpre = 3, target = 6; static constexpr bool regs = true; };
template <> struct RowwiseConfig<4> { static constexpr int kpre = 3, target = 8; static constexpr bool regs = true; };
// Five to eight fields (one pass over the records for up to eight volumes of the same geometry: batch.VolumeBatch)
template <> struct RowwiseConfig<5> { static constexpr int kpre = 3, target = 8; static constexpr bool regs = true; };
template <> struct RowwiseConfig<6> { static constexpr int kpre = 3, target = 8; static constexpr bool regs = true; };
template <> struct RowwiseConfig<7> { static constexpr int kpre = 3, target = 8; static constexpr bool regs = true; };
template <> struct RowwiseConfig<8> { static constexpr int kpre = 3, target = 12; static constexpr bool regs = true; };

// Byte-mask window entries: the window holds v' = the value, or +0 where the gate is excluded, and one BYTE per field that is
// 1 / 0 = usable / excluded.  A pair then costs, per field, half a packed multiply and half a packed add (sum w*v': w * +0 = +0,
// what select + v_mul_legacy_f32 gave), a byte -> float conversion and half a packed fma (sum w*g: the product is exact, so the
// same float32 as adding w or +0) instead of compare + select + v_mul_legacy_f32 + two half packed adds -- the same bits from
// fewer instructions.  Three fields: the mask word is the entry's fourth slot (16-byte entries); four fields: a second array of
// words behind the 16-byte value entries; five to eight fields: 32-byte value entries and two mask words per entry behind them.
// Measured with the pairs of a record taken one at a time (the asm fences of the kernel; without them the wider entries
// cost a wavefront per SIMD and the gain): three / four fields -4 ... -5 % on the bench grid, -1 ... -4 % on config 2
// (19 % fewer VALU instructions: profiles/r04_bytemask_*.json); five fields and more have no other form.
template <int NF> constexpr bool rowwise_bytemask() { return NF >= 3; }
// 4-byte words of LDS per window entry of the row-wise kernel: values, then masks
template <int NF> constexpr int rowwise_value_words() {
  return rowwise_bytemask<NF>() ? (NF <= 4 ? 4 : 8) : 2;     // one field: (v', m); two fields: the two values
}
template <int NF> constexpr int rowwise_mask_words() { return !rowwise_bytemask<NF>() || NF == 3 ? 0 : NF == 4 ? 1 : 2; }
template <int NF> constexpr int rowwise_entry_words() { return rowwise_value_words<NF>() + rowwise_mask_words<NF>(); }


// ---- column mode of the row-wise kernel (rg_csr_compact_apply_columns_f32) --------------------------------------------------
struct ColumnBest {
  float v;     // NaN = nothing seen yet
  int idx;     // -1 = nothing seen yet
};

// np.fmax.reduce in level order (rg_products.hip: step<true>): the first non-NaN level starts the reduction, a later one
// replaces it only when strictly greater; NaN never wins.
__device__ __forceinline__ void column_max_step(ColumnBest& acc, float v, int z) {
  if (acc.idx < 0) {
    if (!isnan(v)) { acc.v = v; acc.idx = z; }
  } else {
    const bool keep = acc.v >= v || isnan(v);
    if (!keep) { acc.v = v; acc.idx = z; }
  }
}

// np.fmin.reduce in level order without the index (rg_products.hip: step<false>): NaN = nothing seen yet, so the first non-NaN
// level starts the reduction and a later one replaces it only when strictly smaller
__device__ __forceinline__ void column_min_step(float& acc, float v) {
  const bool keep = acc <= v || isnan(v);
  if (!keep) acc = v;
}

}  // namespace

// Called across translation units: the tile kernel over the records, 1-4 fields (rg_csr_compact_apply_packed_f32 with tile = 384;
// defined next to the kernel in rg_csr_compact.hip, called from rg_csr_rowwise.hip); `a` and `cg` have passed check_stream_args.
int rg_launch_tile_packed(const rgl::StreamArgs& a, const rgl::ChunkGrid& cg);
