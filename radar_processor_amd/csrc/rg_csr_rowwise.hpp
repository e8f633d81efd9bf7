// The row-wise kernel over the packed records of the compact CSR copy (layout: head of rg_csr_compact.hip; record codings and
// per-field-count tuning: rg_compact_layout.hpp) and its launcher.  A header, so that its modes compile side by side: the grid
// mode in rg_csr_rowwise.hip, the column and planes modes in rg_csr_columns.hip.
#pragma once

#include "rg_compact_layout.hpp"

// ---------------------------------------------------------------------------------------------------------------
// Row-wise kernel over the packed stream (1-4 fields): the default of rg_csr_compact_apply_packed_f32.
// The tile kernel (rg_csr_compact.hip) moves every pair through LDS twice (the product side writes the tile, the row side reads it
// back): 8 bytes per pair each way for one field, 16 + 16 for three on top of the window gather, and from two fields on
// it is LDS- and latency-bound, not HBM-bound.  A packed record already holds three CONSECUTIVE
// pairs, so here the lanes of a row read the row's records straight from memory -- L = 2^k lanes per row, lane j takes
// records q0 + j, q0 + j + L, ... of the row's record range [rs / 3, ceil(re / 3)) -- and reduce them in registers: no
// tile, no transposition; LDS carries only the window gathers.  64 / L rows share a wave-load (L * 16 -- dense coding: L * 14 -- contiguous bytes
// each, neighbouring rows adjacent in memory); a record that straddles two rows is read by both (an L1 hit) and each
// takes its own pairs.  Pairs outside the lane's row are redirected to a sentinel window entry whose slots are all
// EXCLUDED, so the arithmetic needs no extra test.
// A STEP is one batch of KPRE record loads per lane; the loads of the next step (of the same rows, or of the next
// 64 / L rows) are always requested before the current step is summed -- two register stages, as in the tile kernel.
// Summation order (fixed by the geometry and the field count alone, so results are reproducible run to run, on any
// window size and on the per-pair path of an over-wide chunk): a lane's t-th record of a row (t = 0, 1, ...) sits in
// batch slot t mod KPRE and belongs to chain (t mod KPRE) mod 2; per lane and chain, the chain's records in ascending
// order and a record's pairs in order, one running (sum w*v, sum w) per field; chain 0 + chain 1; then the xor butterfly
// of rg_row_phase.hpp over the L lanes.
// L is chosen per segment from its mean row length (kTarget records per lane and row).  This is NOT the order of
// rg_csr_apply_f32: the two agree to float32 rounding, not bit for bit (the tile kernel over the same records, tile =
// 384, does).
// Per field count (measured on config 2 and the bench grid, profiles/r02_rowwise_sweep.json; three fields re-tuned in
// round 3 after the instruction diet of the loop: 3 records per step instead of 2, -2 %, profiles/r03_cfg3_sweep.json):
//   KPRE   records per lane and step;   kTarget  records per lane and row L aims for;
//   kRegs    the row sums travel to lane == row by shuffle and wait in registers instead of an LDS array;
//   one field: the window holds (value, 1) per gate, (0, 0) where it is excluded, and a pair contributes w * (v', m) --
//            the same float32 values as selecting on the sentinel, in packed multiply / add instructions.
// ---------------------------------------------------------------------------------------------------------------
namespace {

constexpr int kRowwiseChunksPerBlock = 1;   // consecutive chunks one workgroup takes (see the kernel: 1 measured best)

// Workgroups per CU the compiler must leave room for (= wavefronts per SIMD: a workgroup is one wavefront per SIMD); 1 = no
// constraint, which is what the row-wise kernel itself measured best with.  How many the hardware then ADMITS is decided by
// two register files, not by VGPRs alone (EXPERIMENTS R5.3): 512 / (VGPR allocation rounded up to 8) wavefronts per SIMD, and
// min(8, 800 / (ceil(.sgpr_count / 16) * 16 + 16)) 256-thread workgroups per CU -- .sgpr_count <= 80 admits eight, <= 96
// seven, anything above six, whatever the compiler's Occupancy remark says.  COLS == 0, one field (what bench.py times): 64
// VGPRs and 94 SGPRs since the grid mode has no chunk loop, so SEVEN workgroups per CU are resident (measured: 6.55 wavefronts
// per SIMD of a busy CU against 5.65 before).  A bound of 7 to hold it there, and a bound of 8 with amdgpu_num_sgpr(80) (62
// VGPRs, 78 SGPRs, 7.47 resident), measured no faster than no bound at all, so it has none.
// COLS == 2 (planes mode): the wider epilogue is
// held to the column mode's wavefronts per SIMD for two to four fields (5, 4, 4) and to at least 5 for one field.  Measured
// (-Rpass-analysis=kernel-resource-usage, no scratch): 80 / 90 / 112 / 120 VGPRs for 1-4 fields, i.e. 6 / 5 / 4 / 4
// wavefronts per SIMD -- the column mode's 77 / 83 / 101 / 107 keep the same counts.
// COLS == 0, four to six fields: 95 VGPRs before the records had two codings, 97 with the second streaming loop left to itself
// -- one register over the 96 that five wavefronts per SIMD allow --, so these three are held to five (no scratch either way).
#define RG_ROWWISE_BOUNDS __launch_bounds__(64 * kH, (COLS == 2 ? (NF <= 2 ? 5 : 4) : (COLS == 0 && NF >= 4 && NF <= 6) ? 5 : 1))
// COLS (rg_csr_compact_apply_columns_f32, csrc/rg_csr_columns.hip): the chunks a workgroup takes one after the other are
// not consecutive blocks of the dispatch order but the LEVELS of one column of chunks -- the same (line group, segment)
// patch from plane z0 to z1 - 1 of its level piece -- so that lane == row sees the voxels of its (y, x) column in ascending
// level order and can keep the column maximum / first argmax in registers and store selected levels as planes; `out`
// may then be null (products only: the 3-D grid is never written).  Everything between a chunk's row pointers and its
// row sums is the same code: the same bits.
// COLS = 1: the column mode; COLS = 2, PLANES (rg_csr_compact_apply_planes_f32, csrc/rg_csr_columns.hip): the column mode
// with the wider epilogue -- per field the
// running minimum and the float32 sum + count of the mean next to the maximum, and up to RG_MAX_SEL_PLANES per-pixel level
// selections whose levels lane == row stores as samples.  Only `if constexpr (PLANES)` code and a kernel argument of its own
// (RowwisePlanes), so the column mode itself compiles to what it was.
// REGS: where the row sums wait for lane == row -- -1 = the field count's default (RowwiseConfig<NF>::regs), 0 = the LDS
// array, 1 = registers.  Four fields: registers cost 99 VGPRs (4 wavefronts per SIMD), the LDS array 95 (5 wavefronts) and
// 8 KiB of LDS per workgroup -- the launcher picks the array wherever the LDS still admits five workgroups per CU.
template <typename IndT, int NF, int STRIDE, int COLS = 0, int REGS = -1>
__global__ RG_ROWWISE_BOUNDS void csr_compact_rowwise_kernel(
    const IndT* __restrict__ indptr, const int64_t* __restrict__ dict_ptr, const int32_t* __restrict__ dict, ChunkGrid cg,
    const float* __restrict__ packed, unsigned last_gate, float fill, int window_cap, long n_vox, float* __restrict__ out,
    const rg_u32x4* __restrict__ rec, const int64_t* __restrict__ rec_ptr, unsigned w_base, int lanes_hint,
    int rec_order, unsigned n_chunks, int chunks_per_block, const std::conditional_t<COLS == 2, RowwisePlanes, RowwiseColumns> cols,
    const uint16_t* __restrict__ row_end16) {
  static_assert(NF >= 1 && NF <= 8 && STRIDE == stride_for(NF), "passes of 1-8 fields");
  constexpr bool PLANES = COLS == 2;
  static_assert(!PLANES || NF <= 4, "the planes mode is the column mode of 1-4 fields");
  using Cfg = RowwiseConfig<NF>;
  constexpr int KPRE = Cfg::kpre;
  constexpr bool kByteMask = rowwise_bytemask<NF>();       // window entries = (v' ..., byte mask): rg_compact_layout.hpp
  constexpr bool kRegs = REGS < 0 ? Cfg::regs : REGS != 0;
  // Five fields and more (never the column mode): a row's sums do not travel to lane == row and wait there (2 * NF registers
  // for the whole segment) -- when a round ends the L lanes of a row, which all hold all its sums after the butterfly, SHARE
  // the fields: lane `sub` divides fields sub, sub + L, ... (a select tree over the bits of sub picks them) and parks the VALUES
  // in 2 KiB of LDS per wavefront; lane == row stores them as whole row runs when the segment ends (storing per round wrote 16-32-row
  // pieces: 1.37x the grid's bytes in partial lines, +1.4 %).  The same sums, the same division: the same bits.
  constexpr bool kScatter = NF >= 5 && !COLS;        // three / four fields: measured slower (stores of 16 rows x 4 fields)
  constexpr int kFenceMinNF = 3;
  // one field: the window holds (v', m) = (value, 1) of a gate, (0, 0) where it is excluded, so that a pair contributes
  // w * (v', m) -- the same float32 values as selecting on the EXCLUDED sentinel (w * 0 = +0, w * 1 = w) in two packed
  // instructions instead of a compare, two selects, a product and two adds
  constexpr bool kPremask = NF == 1;
  extern __shared__ __attribute__((aligned(16))) float window[];   // window_cap + 1 entries of rowwise_entry_words<NF>() words
  // byte masks of four fields and more: the mask words of the window_cap + 1 entries lie behind their value entries
  constexpr int kVW = rowwise_value_words<NF>(), kMW = rowwise_mask_words<NF>();
  // the mask byte of a usable field: the fp8 (OCP e4m3) code of 1.0, read back two fields at a time with v_cvt_pk_f32_fp8
  // (one conversion per field pair instead of a v_cvt_f32_ubyteN per field)
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "the byte masks assume v_cvt_pk_f32_fp8 decodes OCP e4m3 (0x38 = 1.0), as on gfx950"
#endif
  constexpr unsigned kMaskOne = 0x38u;
  (void)kMW;
  unsigned* const maskw = reinterpret_cast<unsigned*>(window + (size_t)(window_cap + 1) * kVW);
  __shared__ f32x2 rowacc_all[kRegs ? 1 : kH][kRegs ? 2 : 64 * NF];
  // kScatter with kStage: the finished values of a segment wait in LDS ([row][8 fields], 2 KiB per wavefront) so that lane == row
  // stores whole 248-byte row runs per field at the segment's end instead of 16-32-row pieces per round
  constexpr bool kStage = kScatter;
  __shared__ __attribute__((aligned(16))) float stage_all[kStage ? kH : 1][kStage ? 64 * 8 : 4];

  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  f32x2* rowacc = rowacc_all[kRegs ? 0 : wv];
  float* const stage = stage_all[kStage ? wv : 0];
  // 26-bit weight mask in a VGPR the compiler cannot fold: (x & mask) | w_base is then ONE v_and_or_b32 (this ISA's VOP3
  // takes no literal, and a literal mask splits it into v_and + v_or)
  unsigned wmask = 0x3FFFFFFu;
  asm volatile("" : "+v"(wmask));

  // A workgroup takes chunks_per_block CONSECUTIVE blocks of the dispatch order, one after the other (the launcher passes 1).
  // Round-3 experiment (EXPERIMENTS.md): the kernel's only store costs 5-15 % of the launch (7.4 ms without it,
  // 7.8-8.7 with it, depending on where records and grid lie in memory), and the first suspect was its acknowledgement
  // at the end of every workgroup's life.  Letting it overlap the next chunk's work changed nothing (2 / 4 / 8 / 32
  // chunks per workgroup: +0.1 ... +0.3 ms, the extra barrier): the cost is the memory system's, a trickle of writes
  // among the reads (tools/exp_placement5.py reproduces it with a bare read probe).
  // COLS: this workgroup's column piece (item = piece * columns + column; columns rotated per line group like the blocks of
  // the dispatch order, so that consecutive workgroups -- consecutive XCDs -- do not pin a column of the grid to one XCD)
  unsigned col_yg = 0, col_sx = 0, col_piece = 0;
  int col_z0 = 0;
  ColumnBest best[COLS ? NF : 1];
  // PLANES: running minimum, float32 sum and count of the mean (per field)
  float pmin[PLANES ? NF : 1], psum[PLANES ? NF : 1];
  int pcnt[PLANES ? NF : 1];
  if constexpr (PLANES) {
#pragma unroll
    for (int f = 0; f < NF; ++f) { pmin[f] = __builtin_nanf(""); psum[f] = 0.0f; pcnt[f] = 0; }
  }
  if constexpr (COLS) {
    const unsigned item = cols.order ? (unsigned)cols.order[blockIdx.x] : blockIdx.x;
    col_piece = item / cols.n_cols;
    const unsigned q = item - col_piece * cols.n_cols;
    col_yg = q / cg.nsx;
    const unsigned c = q - col_yg * cg.nsx;
    col_sx = c + (col_yg * cg.rot_step) % cg.nsx;
    col_sx = col_sx >= cg.nsx ? col_sx - cg.nsx : col_sx;
    col_z0 = (int)((long)col_piece * cg.n_planes / cols.pieces);
    chunks_per_block = (int)((long)(col_piece + 1) * cg.n_planes / cols.pieces) - col_z0;
#pragma unroll
    for (int f = 0; f < NF; ++f) { best[f].v = __builtin_nanf(""); best[f].idx = -1; }
  }
  long col_xy = 0;                                    // COLS: (y, x) of lane == row, the same on every level
  int col_nrows = 0;
  // Grid mode: the launcher's chunks per workgroup is the compile-time kRowwiseChunksPerBlock, so that with 1 the loop, its
  // counter and the block arithmetic fold away (scalars that would otherwise live across the streaming loops).
  const int n_cb = COLS ? chunks_per_block : kRowwiseChunksPerBlock;
  for (int cb = 0; cb < n_cb; ++cb) {
  unsigned bid, chunk;
  if constexpr (COLS) {
    const unsigned grp = (unsigned)(col_z0 + cb) * cg.nyg + col_yg;
    chunk = grp * cg.nsx + col_sx;
    const unsigned shift = ((grp + cg.grp0) * cg.rot_step) % cg.nsx;      // the block whose rotated column is col_sx
    bid = grp * cg.nsx + (col_sx >= shift ? col_sx - shift : col_sx + cg.nsx - shift);
  } else {
    bid = blockIdx.x * (unsigned)kRowwiseChunksPerBlock + (unsigned)cb;
    if (bid >= n_chunks) break;                       // workgroup-uniform
    chunk = block_chunk(cg, bid);
  }
  // Grid mode, dispatch order: a chunk without a record.  The workgroup's kH segments occupy slots bid * kH .. bid * kH + kH - 1 of
  // rec_ptr and a segment without pairs takes no unit, so equal ends mean that no row of the chunk has a neighbour (30 % of the
  // bench grid's chunks: the corners beyond the range, the cone above the top sweep).  Every wavefront stores `fill` to its
  // rows and is done: no dictionary, no row pointers or row ends, no window, no barrier -- the test reads two entries of
  // rec_ptr at addresses that depend on the block alone, so it is WORKGROUP-UNIFORM: all four wavefronts skip the barrier
  // below together, or none does.  (The column and planes modes keep their path: their epilogue runs on these values.)
  if constexpr (!COLS) {
    if (rec_order == RG_REC_ORDER_DISPATCH && rec_ptr[(long)bid * kH] == rec_ptr[((long)bid + 1) * kH]) {
      const Segment se = chunk_segment(cg, chunk, wv);
      if (lane < se.nrows) {
#pragma unroll
        for (int f = 0; f < NF; ++f) out[(size_t)f * n_vox + se.r0 + lane] = fill;
      }
      continue;
    }
  }
  if (cb > 0) __syncthreads();                        // every wavefront is done with the previous chunk's window
  float mine_p[NF], mine_w[NF];                       // kRegs: lane == row
#pragma unroll
  for (int f = 0; f < NF; ++f) mine_p[f] = mine_w[f] = 0.0f;

  const long d0 = dict_ptr[chunk];
  const int nd_all = (int)(dict_ptr[chunk + 1] - d0);
  const bool split = nd_all > 65536;
  const bool windowed = nd_all <= window_cap;        // the window holds window_cap + 1 entries: the sentinel
  // (a split chunk's per-wavefront dictionary window -- w_lo, w_hi -- is read where the per-pair path needs it: run(); the
  // window fill never sees a split chunk, whose dictionary is wider than any window)

  const Segment sg = chunk_segment(cg, chunk, wv);
  const int nrows = sg.nrows;
  const long r0 = sg.r0;
  // Where the rows of the segment begin and end among its pairs: rs_o / re_o of lane == row (a lane past the last row: both
  // = span).  With the row-end table (rg_csr_row_ends16: row_end16[v] = indptr[v + 1] - indptr[r0], two bytes per row instead
  // of indptr's two 8-byte reads) a row begins where the previous one ended, the first at 0, and the span is the last row's
  // end; a segment whose span does not fit carries RG_ROW_END16_WIDE in its last entry and reads indptr as before.  Lanes
  // past the last row read the last entry, so lane 63 holds it whatever nrows is: the choice is wave-uniform, and the 16-bit
  // path reads no indptr.  Both paths hand on the same integers.
  int span = 0, rs_o = 0, re_o = 0;
  unsigned e16 = RG_ROW_END16_WIDE;
  if (row_end16 && nrows) e16 = row_end16[r0 + (lane < nrows ? lane : nrows - 1)];
  if (__builtin_amdgcn_readlane((int)e16, 63) != (int)RG_ROW_END16_WIDE) {
    re_o = (int)e16;
    rs_o = __builtin_amdgcn_update_dpp(0, (int)e16, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);   // lane 0 keeps the 0
    span = __builtin_amdgcn_readlane((int)e16, 63);
  } else if (nrows) {
    const long seg_b = (long)indptr[r0];
    span = (int)((long)indptr[r0 + nrows] - seg_b);
    rs_o = (int)((long)indptr[r0 + (lane < nrows ? lane : nrows)] - seg_b);
    re_o = (int)((long)indptr[r0 + (lane + 1 < nrows ? lane + 1 : nrows)] - seg_b);
  }
  long rec_b = 0, rec_n = 0;
  if (nrows) {
    // dispatch order: the H segments of a workgroup's chunk are neighbours in the stream, and so are consecutive blocks
    const long slot = rec_order == RG_REC_ORDER_DISPATCH ? (long)bid * kH + wv : sg.seg;
    rec_b = rec_ptr[slot];
    rec_n = rec_ptr[slot + 1] - rec_b;
  }
  const rsrc_t rr = make_rsrc(rec + rec_b, rec_n * 16);      // rec_ptr counts 16-byte units in both codings
  // the coding of this chunk's records (rg_compact_layout.hpp): 14 bytes each in a chunk of at most 2048 gates, else 16
  const bool dense = rec_is_dense(nd_all);
  constexpr int kOutOfRange = 0x7FFFFFF0;            // byte offset no segment reaches: the load returns zeros

  // ---- lanes per row ------------------------------------------------------------------------------------------
  int lgl;
  if (lanes_hint > 0 && lanes_hint <= 64) {
    lgl = 31 - __builtin_clz(lanes_hint);
  } else {
    const int target = lanes_hint > 70 ? lanes_hint - 70 : Cfg::target;   // records per lane and row to aim for
    const int mean_rec = nrows ? span / (3 * nrows) + 1 : 1;      // records a row touches, about
    const int need = (mean_rec + target - 1) / target;
    lgl = need <= 1 ? 0 : 32 - __builtin_clz(need - 1);
  }
  lgl = __builtin_amdgcn_readfirstlane(lgl > 6 ? 6 : lgl);
  const int nl = 1 << lgl, rpr = 64 >> lgl;          // lanes per row, rows per round
  const int sub = lane & (nl - 1), rgrp = lane >> lgl;
  const int rounds = (nrows + rpr - 1) >> (6 - lgl);
  // trips of a round = the most records any of its rows gives one lane; lane == row here, groups of rpr rows
  const unsigned q0_row = (unsigned)rs_o / 3u;
  const unsigned q1_row = re_o > rs_o ? ((unsigned)re_o + 2u) / 3u : q0_row;
  int trips_row = (int)((q1_row - q0_row + (unsigned)nl - 1u) >> lgl);
  for (int m = 1; m < rpr; m <<= 1) {
    const int o = __shfl_xor(trips_row, m, 64);
    trips_row = o > trips_row ? o : trips_row;
  }

  // ---- the chunk's field window + the sentinel entry ----------------------------------------------------------
  // kFillBatch entries per thread at a time: their dictionary reads are issued back to back, then their field gathers, then
  // the LDS stores -- two memory latencies per batch.  (Round 2 walked the entries one by one: dictionary read, wait, gather,
  // wait, store -- 2 x 6 serialized latencies in front of the barrier on config 2's 1500-entry dictionaries; other
  // workgroups of the CU cover most of that, the batches are worth 2-5 % there.)  All loads are unconditional on clamped
  // indices so that nothing splits the batch.  Also tried around this prologue in round 3, both slower: issuing the first
  // step's record loads in front of the fill and holding them across it (+22 VGPRs, a wavefront of occupancy: 7-17 %
  // slower), and throw-away loads of the same addresses to warm the L2 meanwhile (+1.4-2.8 %).
  if (windowed) {
    constexpr int kFillBatch = 4;                // 1 / 2 / 8 measured: +2 % / +0.3 % / +0.5 % on config 2 (A/B builds)
    const int last_entry = nd_all > 0 ? nd_all - 1 : 0;
    const int32_t* __restrict__ cd = nd_all > 0 ? dict + d0 : (const int32_t*)dict_ptr;   // never dereference an empty dictionary
    for (int i0 = threadIdx.x; i0 <= nd_all; i0 += 64 * kH * kFillBatch) {
      unsigned gate[kFillBatch];
#pragma unroll
      for (int u = 0; u < kFillBatch; ++u) {
        const int i = i0 + u * 64 * kH;
        gate[u] = (unsigned)cd[i < last_entry ? i : last_entry];
      }
      float v[kFillBatch][STRIDE];
#pragma unroll
      for (int u = 0; u < kFillBatch; ++u) rg::load_packed<STRIDE>(packed, gate[u] < last_gate ? gate[u] : last_gate, v[u]);
#pragma unroll
      for (int u = 0; u < kFillBatch; ++u) {
        // branch-free: a thread past the end stores the sentinel into the sentinel's entry once more (same bits from every
        // such thread), so that nothing conditional makes the compiler sink one of the batch's loads behind a wait
        const int i_raw = i0 + u * 64 * kH;
        const int i = i_raw < nd_all ? i_raw : nd_all;
        if (i_raw >= nd_all) {                   // the sentinel entry: every slot EXCLUDED
#pragma unroll
          for (int s = 0; s < STRIDE; ++s) v[u][s] = __builtin_bit_cast(float, RG_EXCLUDED_BITS);
        }
        if constexpr (kByteMask) {
          unsigned m[2] = {0u, 0u};
          float vv[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
          for (int f = 0; f < NF; ++f) {
            const bool good = rg::f32_bits(v[u][f]) != RG_EXCLUDED_BITS;
            vv[f] = good ? v[u][f] : 0.0f;
            m[f >> 2] |= good ? (kMaskOne << (8 * (f & 3))) : 0u;
          }
          if constexpr (NF == 3) {
            reinterpret_cast<f32x4*>(window)[i] = (f32x4){vv[0], vv[1], vv[2], __builtin_bit_cast(float, m[0])};
          } else if constexpr (NF == 4) {
            reinterpret_cast<f32x4*>(window)[i] = (f32x4){vv[0], vv[1], vv[2], vv[3]};
            maskw[i] = m[0];
          } else {
            reinterpret_cast<f32x4*>(window)[2 * i] = (f32x4){vv[0], vv[1], vv[2], vv[3]};
            reinterpret_cast<f32x4*>(window)[2 * i + 1] = (f32x4){vv[4], vv[5], vv[6], vv[7]};
            reinterpret_cast<uint2*>(maskw)[i] = make_uint2(m[0], m[1]);
          }
        } else if constexpr (kPremask) {
          const bool good = rg::f32_bits(v[u][0]) != RG_EXCLUDED_BITS;
          reinterpret_cast<f32x2*>(window)[i] = good ? (f32x2){v[u][0], 1.0f} : (f32x2){0.0f, 0.0f};
        } else {                                 // two fields
          reinterpret_cast<f32x2*>(window)[i] = (f32x2){v[u][0], v[u][1]};
        }
      }
    }
  }
  __syncthreads();

  // A STEP is one batch of KPRE record loads per lane: batch b of round rho.  A round whose rows need more than KPRE
  // trips simply takes several steps, so every load of the kernel is requested one step ahead whatever the row lengths.
  // Per-step lane state is kept in the form the loop consumes it, so that a record costs one add and one compare to
  // place: batch slot k of a step holds the lane's record number q + k * L.
  struct Step {
    int lo0;           // (first pair of the lane's row) - 3 * q: pair i of slot k is the row's iff 0 <= i - lo < len,
    unsigned len;      //   lo = lo0 - 3 * k * L; len = pairs of the row (0: no row)
    int rem;           // records of the row from q on: slot k holds one iff k * L < rem.  Dense records: 2 * that + (q & 1) --
                       //   k * L < rem iff 2 * k * L + 1 < 2 * rem + parity, so the parity of q rides along for free
    int off0;          // byte offset of record q in the segment's records
    int myrow, rho;
    int left;          // trips of the round still to do, this batch included (wave-uniform)
    bool live;
  };
  auto setup = [&](auto dtag, int rho) -> Step {
    constexpr int rec_bytes = decltype(dtag)::value ? 14 : 16;
    Step r;
    r.rho = rho;
    r.myrow = rho * rpr + rgrp;
    r.live = r.myrow < nrows;
    // both shuffles unconditional: a lane that is dead in this round still has to SUPPLY its row bounds (a shuffle
    // under a divergent condition reads zeros from the lanes that skipped it)
    const int qs = __shfl(rs_o, r.myrow & 63, 64);
    const int qe_row = __shfl(re_o, r.myrow & 63, 64);
    const int qe = r.live ? qe_row : qs;
    const int q0 = (int)((unsigned)qs / 3u);
    const int q1 = qe > qs ? (int)(((unsigned)qe + 2u) / 3u) : q0;
    const int q = q0 + sub;
    r.lo0 = qs - 3 * q;
    r.len = (unsigned)(qe - qs);
    r.rem = decltype(dtag)::value ? 2 * (q1 - q) + (q & 1) : q1 - q;
    r.off0 = q * rec_bytes;
    r.left = rho < rounds ? __builtin_amdgcn_readfirstlane(__shfl(trips_row, (rho * rpr) & 63, 64)) : 0;
    return r;
  };
  auto advance = [&](auto dtag, const Step& r) -> Step {      // the step after r (wave-uniform choice)
    constexpr int rec_bytes = decltype(dtag)::value ? 14 : 16;
    if (r.left > KPRE) {
      Step n = r;
      n.lo0 -= 3 * (KPRE << lgl);
      if constexpr (decltype(dtag)::value) n.rem = (n.rem - 2 * (KPRE << lgl)) ^ ((KPRE << lgl) & 1);   // q + KPRE * L: its parity
      else n.rem -= KPRE << lgl;
      n.off0 += rec_bytes * (KPRE << lgl);
      n.left -= KPRE;
      return n;
    }
    return setup(dtag, r.rho + 1);
  };
  // dense: the aligned 16 bytes that hold the record -- it starts at byte 0 of the load when q is even, at byte 2 when odd
  auto issue = [&](auto dtag, const Step& r, rg_u32x4 (&regs)[KPRE]) {
    constexpr bool kDense = decltype(dtag)::value;
#pragma unroll
    for (int k = 0; k < KPRE; ++k) {
      const int off = kDense ? (r.off0 + 14 * (k << lgl)) & ~3 : r.off0 + 16 * (k << lgl);
      const bool has = kDense ? 2 * (k << lgl) + 1 < r.rem : (k << lgl) < r.rem;
      regs[k] = rg_buffer_load_v4u32(rr, has ? off : kOutOfRange, 0, 0);
    }
  };
  auto run = [&](auto wtag, auto dtag) {
    constexpr bool kWindowed = decltype(wtag)::value;
    constexpr bool kDense = decltype(dtag)::value;
    // per-pair path: the wavefront's part of the chunk's dictionary (a split chunk -- more than 65536 entries -- gives every
    // wavefront a window of its own, whose bounds are the dictionary's first kH entries)
    const int w_lo = !kWindowed && split ? dict[d0 + wv] : 0;
    const int w_hi = !kWindowed && split && wv + 1 < kH ? dict[d0 + wv + 1] : nd_all;
    const int nd_last = w_hi - w_lo > 0 ? w_hi - w_lo - 1 : 0;
    const int32_t* __restrict__ cdict = dict + d0 + w_lo;
    // The running sums of the lane's row, across the round's steps: TWO chains -- batch slot k of every step adds into
    // chain k mod 2's (sum w*v, sum w) --, added up when the round ends.  Two independent chains half as long as round 2's
    // single one: worst relative error against the reference's ZDR fixtures 8.7e-6 -> 6.5e-6 at no cost (bench grid
    // 8.051 vs 8.050 ms, same process and arrays; <= 1.3 % for 2-4 fields).  One chain per slot (three) reaches 4.3e-6 --
    // exact sums would give 4.2e-6, the reference's own rounding -- but costs a wavefront of occupancy (75 -> 89 VGPRs for
    // one field): +2.1 % on the bench grid, +10 / +21 % for two / four fields (profiles/r03_slots_ab.json).
    constexpr int KS = 2;
    // Five fields and more: the weight sums keep ONE chain.  They add positive terms only, so their rounding is a few 1e-8
    // of the sum whatever the order; the products -- where mixed signs cancel and the order shows in the result -- keep two.
    // (Eight fields: 165 VGPRs with two chains each, 3 wavefronts per SIMD; 4 wavefronts need <= 128.)
    constexpr int KSW = NF >= 5 ? 1 : KS;
    // Byte-mask kernels keep the sums of field PAIRS in 64-bit register pairs (bp / bw: what v_pk_mul / v_pk_add / v_pk_fma
    // take, and what the per-pair asm fences can name without splitting the pairs); the others keep scalars the compiler pairs.
    constexpr int NP2 = (NF + 1) / 2;
    float ap[kByteMask ? 1 : KS][kByteMask ? 1 : NF], aw[kByteMask ? 1 : KSW][kByteMask ? 1 : NF];
    f32x2 bp[kByteMask ? KS : 1][kByteMask ? NP2 : 1], bw[kByteMask ? KSW : 1][kByteMask ? NP2 : 1];
#pragma unroll
    for (int k = 0; k < (kByteMask ? 1 : KS); ++k) {
#pragma unroll
      for (int f = 0; f < (kByteMask ? 1 : NF); ++f) ap[k][f] = 0.0f;
    }
#pragma unroll
    for (int k = 0; k < (kByteMask ? 1 : KSW); ++k) {
#pragma unroll
      for (int f = 0; f < (kByteMask ? 1 : NF); ++f) aw[k][f] = 0.0f;
    }
#pragma unroll
    for (int k = 0; k < (kByteMask ? KS : 1); ++k) {
#pragma unroll
      for (int j = 0; j < (kByteMask ? NP2 : 1); ++j) bp[k][j] = (f32x2)(0.0f);
    }
#pragma unroll
    for (int k = 0; k < (kByteMask ? KSW : 1); ++k) {
#pragma unroll
      for (int j = 0; j < (kByteMask ? NP2 : 1); ++j) bw[k][j] = (f32x2)(0.0f);
    }
    auto addp = [&](int k, int f, float x) {          // k, f compile-time after unrolling
      if constexpr (kByteMask) bp[k][f >> 1][f & 1] += x; else ap[k][f] += x;
    };
    auto addw = [&](int k, int f, float x) {
      if constexpr (kByteMask) bw[k][f >> 1][f & 1] += x; else aw[k][f] += x;
    };
    auto fence_sums = [&](int kp, int kw) {           // everything added so far is complete; no memory access moves across
      if constexpr (kByteMask) {
#pragma unroll
        for (int j = 0; j < NP2; ++j) asm volatile("" : "+v"(bp[kp][j]), "+v"(bw[kw][j]) : : "memory");
      } else {
#pragma unroll
        for (int f = 0; f < NF; ++f) asm volatile("" : "+v"(ap[kp][f]), "+v"(aw[kw][f]) : : "memory");
      }
    };
    auto consume = [&](const Step& r, const rg_u32x4& q4, int k) {     // k: slot of the step's batch (compile-time)
      // The record's pairs i = 0, 1, 2 belong to the lane's row iff lo <= i < lo + len, lo = lo0 - 3 * k * L.  Taken against
      // wave-uniform constants: 3 * k * L + i < lo0 + len, and lo0 <= i where that can fail at all -- lo0 = (first pair mod 3)
      // - 3 * sub <= 2 in a row's first step and lower in every later one, so only pairs 0 and 1 of slot 0 need the test.  A
      // slot past the row's last record needs no test of its own (issue() keeps one: its loads are real bytes): its pairs'
      // numbers in the segment are >= 3 * ceil(row end / 3) >= the row's end; a lane without a row has len = 0.
      // (tests/test_rowwise_prologue_scenes.py holds this against the definition.)
      const int hi = r.lo0 + (int)r.len;
      float w[3];
      int pos[3];
      // dense: bit 0 of rem is the parity of q; the record's number is q + k * L (k * L is odd only for odd k and L = 1)
      const RecFields rf = rec_decode<kDense>(q4, !kDense ? 0u : (k & 1) ? (unsigned)r.rem ^ (unsigned)(k << lgl) : (unsigned)r.rem);
      // w_base has its low 26 bits clear (the entry point checks), so code | w_base == code + w_base
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        w[i] = __builtin_bit_cast(float, (rf.wc[i] & wmask) | w_base);
        pos[i] = (int)rf.pos[i];
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const bool mine = 3 * (k << lgl) + i < hi && (k > 0 || i == 2 || r.lo0 <= i);
        // windowed: no clamp -- a position is 16 bits by construction, and an LDS read beyond the workgroup's allocation
        // returns zeros instead of faulting (a corrupt record cannot do worse than a wrong value)
        const int p = kWindowed ? pos[i] : (pos[i] < nd_last ? pos[i] : nd_last);
        float v[STRIDE];
        if constexpr (kWindowed) {
          const int e = mine ? p : nd_all;          // not this row's pair: the all-EXCLUDED sentinel entry
          __builtin_assume((unsigned)e <= 65536u);  // lets e * 12 be a 24-bit multiply-add instead of a 64-bit one
          if constexpr (kByteMask) {
            // (v', byte mask): sum w*v' by multiply + add (w * +0 = +0 where excluded, as the select + legacy multiply gave),
            // sum w*g by fma (exact product: the same float32 as adding w or +0)
            float vv[8];
            unsigned m[2] = {0u, 0u};
            if constexpr (NF <= 4) {
              const f32x4 x = reinterpret_cast<const f32x4*>(window)[e];
              vv[0] = x.x; vv[1] = x.y; vv[2] = x.z; vv[3] = x.w;
              m[0] = NF == 3 ? rg::f32_bits(x.w) : maskw[e];
            } else {
              const f32x4 x = reinterpret_cast<const f32x4*>(window)[2 * e], y = reinterpret_cast<const f32x4*>(window)[2 * e + 1];
              vv[0] = x.x; vv[1] = x.y; vv[2] = x.z; vv[3] = x.w; vv[4] = y.x; vv[5] = y.y; vv[6] = y.z; vv[7] = y.w;
              const uint2 mm = reinterpret_cast<const uint2*>(maskw)[e];
              m[0] = mm.x; m[1] = mm.y;
            }
            // one conversion per field PAIR: v_cvt_pk_f32_fp8 (OCP e4m3: 0x38 = 1.0, 0x00 = +0)
            using g2_t = decltype(__builtin_amdgcn_cvt_pk_f32_fp8(0, false));
            const g2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)m[0], false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)m[0], true);
            const g2_t c = __builtin_amdgcn_cvt_pk_f32_fp8((int)m[1], false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)m[1], true);
            const f32x2 g2[4] = {(f32x2){a[0], a[1]}, (f32x2){b[0], b[1]}, (f32x2){c[0], c[1]}, (f32x2){d[0], d[1]}};
            const f32x2 w2 = (f32x2){w[i], w[i]};
#pragma unroll
            for (int j = 0; j < NP2; ++j) {
              const f32x2 prod = w2 * (f32x2){vv[2 * j], vv[2 * j + 1]};       // float32 product, then the add (no contraction)
              bp[k % KS][j] += prod;
              bw[k % KSW][j] = __builtin_elementwise_fma(w2, g2[j], bw[k % KSW][j]);
            }
            if constexpr (NF >= kFenceMinNF) fence_sums(k % KS, k % KSW);   // one pair at a time: these sums are complete
            continue;                                                       // before the next pair's window reads are issued
          } else if constexpr (kPremask) {
            const f32x2 term = (f32x2){w[i], w[i]} * reinterpret_cast<const f32x2*>(window)[e];
            ap[k % KS][0] += term.x;
            aw[k % KSW][0] += term.y;
            continue;
          } else {                                  // two fields
            const f32x2 x = reinterpret_cast<const f32x2*>(window)[e];
            v[0] = x.x; v[1] = x.y;
          }
        } else {
          const unsigned g0 = (unsigned)cdict[p];
          rg::load_packed<STRIDE>(packed, g0 < last_gate ? g0 : last_gate, v);
          if (!mine) {
#pragma unroll
            for (int s = 0; s < STRIDE; ++s) v[s] = __builtin_bit_cast(float, RG_EXCLUDED_BITS);
          }
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) {   // masked gate: contributes to neither sum (interpolate.py:78-79)
          const bool good = rg::f32_bits(v[f]) != RG_EXCLUDED_BITS;
          // ONE select per field and pair: the effective weight is w or +0, and v_mul_legacy_f32 makes 0 * sentinel = +0
          // where an IEEE multiply would make NaN (for a non-zero weight the two multiplies are the same operation, so
          // unmasked NaN / Inf data propagates exactly as before: same bits as good ? w * v : 0)
          const float wf = good ? w[i] : 0.0f;
          addp(k % KS, f, rg_fmul_legacy(wf, v[f]));
          addw(k % KSW, f, wf);
        }
        // the per-pair path of an over-wide chunk (rare): five fields and more take its pairs one at a time -- three 32-byte
        // gathers in flight per record would set the whole kernel's register count (167 instead of <= 128 for eight fields)
        if constexpr (NF >= kFenceMinNF) fence_sums(k % KS, k % KSW);
      }
    };
    // sums of step r's batch; `last`: the round ends here -> fold the row's lanes and hand the sums to the row
    auto process = [&](const Step& r, const rg_u32x4 (&regs)[KPRE], bool last) {
#pragma unroll
      for (int k = 0; k < KPRE; ++k) {
        if (k < r.left) consume(r, regs[k], k);   // wave-uniform
      }
      if (!last) return;
      float sv[2 * NF];
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        float sp, sw;                                  // chains in ascending order
        if constexpr (kByteMask) {
          sp = bp[0][f >> 1][f & 1];
          sw = bw[0][f >> 1][f & 1];
#pragma unroll
          for (int k = 1; k < KS; ++k) sp += bp[k][f >> 1][f & 1];
#pragma unroll
          for (int k = 1; k < KSW; ++k) sw += bw[k][f >> 1][f & 1];
        } else {
          sp = ap[0][f];
          sw = aw[0][f];
          ap[0][f] = aw[0][f] = 0.0f;
#pragma unroll
          for (int k = 1; k < KS; ++k) {
            sp += ap[k][f];
            ap[k][f] = 0.0f;
          }
#pragma unroll
          for (int k = 1; k < KSW; ++k) {
            sw += aw[k][f];
            aw[k][f] = 0.0f;
          }
        }
        sv[2 * f] = sp;
        sv[2 * f + 1] = sw;
      }
      if constexpr (kByteMask) {
#pragma unroll
        for (int k = 0; k < KS; ++k) {
#pragma unroll
          for (int j = 0; j < NP2; ++j) bp[k][j] = (f32x2)(0.0f);
        }
#pragma unroll
        for (int k = 0; k < KSW; ++k) {
#pragma unroll
          for (int j = 0; j < NP2; ++j) bw[k][j] = (f32x2)(0.0f);
        }
      }
      rg::butterfly<2 * NF>(sv, nl);
      if constexpr (kScatter) {
        constexpr int NP = NF <= 2 ? 2 : NF <= 4 ? 4 : 8, LGP = NF <= 2 ? 1 : NF <= 4 ? 2 : 3;    // fields, padded to 2^LGP
        float p[NP], w[NP];
#pragma unroll
        for (int f = 0; f < NP; ++f) {
          p[f] = f < NF ? sv[2 * (f < NF ? f : 0)] : 0.0f;
          w[f] = f < NF ? sv[2 * (f < NF ? f : 0) + 1] : 0.0f;
        }
        // after s stages entry j holds field j * 2^s + (sub mod 2^s)
        const int stages = lgl < LGP ? lgl : LGP;                   // wave-uniform
#pragma unroll
        for (int st = 0; st < LGP; ++st) {
          if (st < stages) {
            const bool bit = ((sub >> st) & 1) != 0;
#pragma unroll
            for (int i = 0; i < (NP >> (st + 1)); ++i) {
              p[i] = bit ? p[2 * i + 1] : p[2 * i];
              w[i] = bit ? w[2 * i + 1] : w[2 * i];
            }
          }
        }
        const int lp = 1 << stages;                                 // fields a row's lanes share among themselves
        const int f0 = sub & (lp - 1);
        const bool owner = r.live && (sub >> stages) == 0;          // more lanes per row than (padded) fields: the first store
        float* dst = out + ((size_t)f0 * n_vox + r0 + r.myrow);
        const size_t step_f = (size_t)lp * n_vox;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
          if (j < (NP >> stages)) {                                 // wave-uniform
            if constexpr (kStage) {
              if (owner && f0 + j * lp < NF) stage[r.myrow * 8 + f0 + j * lp] = w[j] > 0.0f ? p[j] / w[j] : fill;
            } else {
              if (owner && f0 + j * lp < NF) dst[j * step_f] = w[j] > 0.0f ? p[j] / w[j] : fill;
            }
          }
        }
      } else if constexpr (kRegs) {      // every lane of a row holds the row's sums: lane == row fetches them
        const int first = r.myrow - rgrp;                   // the round's first row (wave-uniform)
        const bool take = lane >= first && lane < first + rpr;
        const int src = ((lane - first) << lgl) & 63;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          const float gp = __shfl(sv[2 * f], src, 64), gw = __shfl(sv[2 * f + 1], src, 64);
          mine_p[f] = take ? gp : mine_p[f];
          mine_w[f] = take ? gw : mine_w[f];
        }
      } else if (r.live && sub == 0) {
#pragma unroll
        for (int f = 0; f < NF; ++f) rowacc[r.myrow * NF + f] = (f32x2){sv[2 * f], sv[2 * f + 1]};
      }
    };

    rg_u32x4 regs_a[KPRE], regs_b[KPRE];
    Step sa = setup(dtag, 0), sb;
    issue(dtag, sa, regs_a);
    for (;;) {     // two register stages, alternating: nothing in flight is ever copied
      sb = advance(dtag, sa);
      issue(dtag, sb, regs_b);
      process(sa, regs_a, sb.rho != sa.rho);
      if (sb.rho >= rounds) break;
      sa = advance(dtag, sb);
      issue(dtag, sa, regs_a);
      process(sb, regs_b, sa.rho != sb.rho);
      if (sa.rho >= rounds) break;
    }
  };
  if (span > 0) {       // the streaming loop exists once per (window | per-pair gathers) x (dense | wide records): workgroup-uniform
    if (dense) {
      if (windowed) run(std::true_type{}, std::true_type{}); else run(std::false_type{}, std::true_type{});
    } else {
      if (windowed) run(std::true_type{}, std::false_type{}); else run(std::false_type{}, std::false_type{});
    }
  }
  // PLANES: the selection words of lane == row, read again at every level (from L2: 4 bytes per selection and row) rather than
  // kept in registers through the streaming loop, where they would cost two fields a wavefront per SIMD
  // (32-bit pixel offsets from wave-uniform bases: the loads and stores take the scalar-base form, no 64-bit address per lane)
  int psel[PLANES ? RG_MAX_SEL_PLANES : 1];
  unsigned pxy = 0;
  if constexpr (PLANES) {
    pxy = (unsigned)(r0 - (long)(col_z0 + cb) * cols.n_xy) + (unsigned)lane;
#pragma unroll
    for (int s = 0; s < RG_MAX_SEL_PLANES; ++s) psel[s] = (s < cols.n_sel && lane < nrows) ? cols.sel[s][pxy] : RG_PPI_SEL_NONE;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  if constexpr (kStage) {
    if (span > 0 && lane < nrows) {                   // (the wave barrier above orders the rounds' LDS writes before these reads)
      // the lane's staging address is formed here, behind a fence: as a loop invariant it lived in a register from before the
      // first chunk to this read, and six fields, at the 96 registers five wavefronts allow, spilled it to scratch
      int sl = lane;
      asm volatile("" : "+v"(sl));
      const f32x4 lo = reinterpret_cast<const f32x4*>(stage)[2 * sl], hi = reinterpret_cast<const f32x4*>(stage)[2 * sl + 1];
      const float vals[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
      for (int f = 0; f < NF; ++f) out[(size_t)f * n_vox + r0 + lane] = vals[f];
    }
  }
  if (lane < nrows && !(kScatter && span > 0)) {     // kScatter: the rounds stored their rows; a segment without pairs has none
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      f32x2 s = (f32x2)(0.0f);
      if constexpr (kRegs) s = (f32x2){mine_p[f], mine_w[f]};
      else if (span > 0) s = rowacc[lane * NF + f];
      if constexpr (COLS) {
        const float val = s.y > 0.0f ? (float)((double)s.x / (double)s.y) : fill;
        const int z = col_z0 + cb;
        if (out) out[(size_t)f * n_vox + r0 + lane] = val;
        if (cols.planes && z >= cols.keep_lo && z < cols.keep_lo + cols.n_keep)
          cols.planes[((size_t)f * cols.n_keep + (z - cols.keep_lo)) * cols.n_xy + (r0 - (long)z * cols.n_xy) + lane] = val;
        if (cols.col_val && z >= cols.col_lo && z <= cols.col_hi) column_max_step(best[f], val, z);
        if constexpr (PLANES) {
          if (z >= cols.col_lo && z <= cols.col_hi) {
            if (cols.col_min) column_min_step(pmin[f], val);
            if (cols.col_mean) {                    // np.nanmean: NaN -> 0, float32 adds in level order (rg_products.hip)
              const bool nan = isnan(val);
              psum[f] = __fadd_rn(psum[f], nan ? 0.0f : val);
              pcnt[f] += nan ? 0 : 1;
            }
          }
#pragma unroll
          for (int s = 0; s < RG_MAX_SEL_PLANES; ++s) {
            if (s < cols.n_sel) {
              float* const smp = cols.samples + ((size_t)(f * cols.n_sel + s) * 2) * cols.n_xy;    // [f][s][0 | 1][pixel]
              if (z == (psel[s] & 0xFFFF)) smp[pxy] = val;
              if (z == (int)((unsigned)psel[s] >> 16)) smp[cols.n_xy + pxy] = val;
            }
          }
        }
      } else {
        out[(size_t)f * n_vox + r0 + lane] = s.y > 0.0f ? (float)((double)s.x / (double)s.y) : fill;
      }
    }
  }
  if constexpr (COLS) {
    col_nrows = nrows;
    col_xy = r0 - (long)(col_z0 + cb) * cols.n_xy + lane;
    if constexpr (!kRegs) {      // the next level's rounds overwrite the row sums in LDS: this level's reads come first
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
  }   // chunks of this workgroup
  if constexpr (PLANES) {
    if (lane < col_nrows) {
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const size_t o = ((size_t)col_piece * NF + f) * cols.n_xy + col_xy;
        if (cols.col_val) {
          cols.col_val[o] = best[f].v;
          if (cols.col_arg) cols.col_arg[o] = best[f].idx;
        }
        if (cols.col_min) cols.col_min[o] = pmin[f];
        if (cols.col_mean) cols.col_mean[o] = (float)((double)psum[f] / (double)pcnt[f]);      // 0 / 0 -> NaN; one piece
      }
    }
  } else if constexpr (COLS) {
    if (cols.col_val && lane < col_nrows) {
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const size_t o = ((size_t)col_piece * NF + f) * cols.n_xy + col_xy;
        cols.col_val[o] = best[f].v;
        if (cols.col_arg) cols.col_arg[o] = best[f].idx;
      }
    }
  }
}

// The three modes launch the same way: the window is cut to what 64 KiB of LDS hold next to `static_lds` bytes of static
// arrays (one entry beyond window_cap: the sentinel; a smaller window only sends more chunks down the per-pair path).
template <typename IndT, int NF, int COLS, int REGS, typename Cols>
int launch_rowwise(const char* fn, const StreamArgs& a, const ChunkGrid& cg, long static_lds, dim3 grid, int chunks_per_block,
                   const Cols& cols) {
  constexpr int WS = rowwise_entry_words<NF>();                                   // 4-byte words per window entry
  const long room = (65536 - static_lds - 256) / (4 * WS) - 1;
  const int window_cap = a.window_cap > room ? (int)room : a.window_cap;
  hipLaunchKernelGGL((csr_compact_rowwise_kernel<IndT, NF, stride_for(NF), COLS, REGS>), grid, dim3(64 * kH),
                     ((size_t)(window_cap + 1) * WS * sizeof(float) + 15) / 16 * 16, a.stream, static_cast<const IndT*>(a.indptr),
                     a.dict_ptr, a.dict, cg, a.packed, (unsigned)(a.n_gates - 1), a.fill, window_cap, a.n_vox, a.out,
                     static_cast<const rg_u32x4*>(a.records), a.rec_ptr, a.w_base, a.lanes_hint, a.rec_order,
                     (unsigned)chunk_count(cg), chunks_per_block, cols, a.row_end16);
  return rg::check_launch(fn);
}

}  // namespace
