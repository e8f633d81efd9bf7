// K1p  rg_csr_compact_apply_columns_f32: the row-wise kernel of rg_csr_rowwise.hpp with workgroups that are PERSISTENT over a
// COLUMN of chunks -- the same (line group, segment) patch through consecutive grid levels -- and an optional products
// epilogue (COLMAX / first-argmax in registers, selected levels stored as planes) that removes the 3-D grid's round trip
// through HBM.  radar_grid/interpolate.py:69-104 (the masked weighted mean), :137-140 (several fields, one pass);
// radar_grid/products.py:361-412 (CAPPI needs two levels), :462-490 (column maximum over a level window).
//
// Why: callers that keep 2-D products only (BASELINE configs 3 and 5) no longer write F x 4 x V bytes of grid and read them
// back -- on this part writes mixed into a streaming read cost ten times their stand-alone price.
//
// The kernel is the COLUMN MODE of the row-wise kernel itself (csr_compact_rowwise_kernel<..., COLS = true> in
// rg_csr_rowwise.hpp): the same code from a chunk's row pointers to its row sums, one chunk after the other behind a barrier,
// with 4-12 more VGPRs for the running maxima.  This file instantiates that mode and the planes mode, and holds their entry
// points and the merge of level pieces.
//
// Measured (round 4, profiles/r04_columns_variants_*.json; ms per pass, bench grid / config 2, same process and arrays):
// products only against row-wise kernel + separate COLMAX/argmax + CAPPI: one field 8.19 vs 8.07 / 1.16 vs 1.01, three
// fields 10.73 vs 10.52 / 1.41 vs 1.40, four fields 11.49 vs 12.03 / 1.53 vs 1.58 -- the store it saves (0.25-0.3 ms per
// pass here) is what walking columns costs (workgroups no longer sweep the grid as one front: neighbouring chunks stop
// sharing their gathers in L2), so it pays from four field-volumes per pass on, and always in memory (no F x 640 MB of grid).
// Two designs that ALSO tried to take the per-chunk chain of dependent loads (row pointers / offsets -> dictionary ->
// gathers -> barrier -> records) off the critical path were built, tested bit-identical and measured slower; they lived in
// this file at commit 54393d1 and are written up in EXPERIMENTS.md:
//   LOADER  a fifth wavefront fills a SECOND LDS window with chunk k+1 and publishes chunk k+2's metadata in an LDS ring while
//           four stream chunk k across the boundary: 1.6-2.6x slower (half the resident streaming wavefronts per CU);
//   WALK    four wavefronts, one window, chunk k+1's metadata held in registers a chunk ahead and its first records
//           requested before the window is filled: +7-11 % (12-36 more VGPRs cost a wavefront per SIMD).
//
// Arithmetic: per row exactly the row-wise kernel's -- same lanes per row (from the segment's mean row length), same
// batches of KPRE records, same two chains per lane, same butterfly, same float64 division -- so the 3-D grid is the same
// BITS as rg_csr_compact_apply_packed_f32 (tile = 0) and as oracle.csr_apply_rowwise_order (tests assert both).
// Products: lane == row of a streaming wavefront sees the levels of its (y, x) column in ascending order, so the column
// maximum follows np.fmax.reduce (first of equal values wins, NaN ignored) and the arg is the first level attaining it,
// -1 for an all-NaN column -- the contract of rg_column_reduce_f32 (csrc/rg_products.hip), bit for bit.  Levels
// [keep_lo, keep_lo + n_keep) are stored as planes (CAPPI's two levels; the caller blends them with rg_cappi_lerp_f32).
// With z_pieces > 1 a column is cut into level ranges handled by different workgroups (more workgroups on small grids);
// the partial (max, arg) planes are merged in ascending level order by a second tiny kernel -- associative, bit-exact.
//
// Roofline: HBM.  Bytes per launch = the row-wise kernel's minus what is not stored: 16*R + 8*(S+1) + 4*D + 8*(C+1) +
// ip*(V+1) + F*5*G + F*4*V [only if out] + F*4*Vxy*(n_keep [+ 2 if colmax]).
#include "rg_csr_rowwise.hpp"

namespace {

// Column mode (Cols = RowwiseColumns) and planes mode (RowwisePlanes: the same launch with the wider epilogue) of the row-wise
// kernel, 1-4 fields: one workgroup per column of chunks and level piece.
template <typename Cols>
int launch_rowwise_cols(const StreamArgs& a, const ChunkGrid& cg, const Cols& cols) {
  constexpr bool PLANES = std::is_same_v<Cols, RowwisePlanes>;
  constexpr int kRegsCols = -1;      // (four fields with the row sums in LDS: 108 instead of 111 VGPRs, the same 4 wavefronts)
  return rg::dispatch_index(a.is_i64, [&](auto ind) {
    return rg::dispatch_fields<4>(a.n_fields, [&](auto nf, auto) {
      constexpr int NF = decltype(nf)::value;
      constexpr long kStatic = RowwiseConfig<NF>::regs ? 16 : (long)kH * 64 * NF * 8;
      return launch_rowwise<decltype(ind), NF, PLANES ? 2 : 1, kRegsCols>(
          PLANES ? "rg_csr_compact_apply_planes_f32" : "rg_csr_compact_apply_columns_f32", a, cg, kStatic,
          dim3(cols.n_cols * (unsigned)cols.pieces), 1, cols);
    });
  });
}

// (max, first arg) of a column from the partial results of its level pieces, merged in ascending level order: a later
// piece wins only when strictly greater (rg_products.hip: merge<true> with b.idx > a.idx)
__global__ __launch_bounds__(256) void columns_merge_kernel(const float* __restrict__ part_val, const int32_t* __restrict__ part_arg,
                                                            int pieces, long n_planes_xy, float* __restrict__ out_val,
                                                            int32_t* __restrict__ out_arg) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_planes_xy) return;
  float v = part_val[i];
  int idx = part_arg[i];
  for (int p = 1; p < pieces; ++p) {
    const float bv = part_val[(size_t)p * n_planes_xy + i];
    const int bi = part_arg[(size_t)p * n_planes_xy + i];
    if (bi >= 0 && (idx < 0 || bv > v)) { v = bv; idx = bi; }
  }
  out_val[i] = v;
  if (out_arg) out_arg[i] = idx;
}

// minimum of a column from the partial minima of its level pieces, merged in ascending level order (rg_products.hip:
// merge<false>): NaN = the piece saw no value; a later piece wins only when strictly smaller
__global__ __launch_bounds__(256) void planes_min_merge_kernel(const float* __restrict__ part_val, int pieces, long n_planes_xy,
                                                               float* __restrict__ out_val) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_planes_xy) return;
  float v = part_val[i];
  for (int p = 1; p < pieces; ++p) {
    const float bv = part_val[(size_t)p * n_planes_xy + i];
    if (!isnan(bv) && (isnan(v) || bv < v)) v = bv;
  }
  out_val[i] = v;
}

}  // namespace

extern "C" int64_t rg_csr_columns_workspace_bytes(int64_t lines_per_plane, int64_t line_len, int32_t n_fields,
                                                  int32_t z_pieces) {
  if (lines_per_plane <= 0 || line_len <= 0 || n_fields < 1 || n_fields > 4 || z_pieces < 1) return RG_EINVAL;
  if (z_pieces == 1) return 0;
  return (int64_t)z_pieces * n_fields * lines_per_plane * line_len * 8;      // partial (max, arg) planes
}

// _ex: with the row-end table of the grid (rg_csr_row_ends16; null = none, what rg_csr_compact_apply_columns_f32 passes)
extern "C" int rg_csr_compact_apply_columns_f32_ex(const void* indptr, int32_t indptr_is_i64, const void* records,
                                                   const int64_t* rec_ptr, int32_t rec_order, uint32_t w_base,
                                                   const int64_t* dict_ptr, const int32_t* dict, int64_t n_vox, int64_t n_pairs,
                                                   int64_t line_len, int64_t lines_per_plane, const float* packed,
                                                   int32_t n_fields, int32_t stride, int64_t n_gates, float fill_value,
                                                   float* out, float* level_planes, int32_t keep_lo, int32_t n_keep,
                                                   float* col_max, int32_t* col_arg, int32_t col_lo, int32_t col_hi,
                                                   int32_t window_cap, int32_t z_pieces, const int32_t* order, void* workspace,
                                                   int64_t workspace_bytes, int32_t lanes_hint, const uint16_t* row_end16,
                                                   rg_stream_t stream) {
  RG_REQUIRE(out || level_planes || col_max, RG_EINVAL,
             "rg_csr_compact_apply_columns_f32: nothing to produce (out, level_planes and col_max are all null)");
  const StreamArgs a{indptr, indptr_is_i64 != 0, records, rec_ptr, rec_order, w_base, dict_ptr, dict, n_vox, n_pairs, line_len,
                     lines_per_plane, packed, n_fields, stride, n_gates, fill_value, out, window_cap, lanes_hint,
                     (hipStream_t)stream, /*max_fields=*/4, /*need_out=*/false, /*need_packed=*/true, row_end16};
  ChunkGrid cg;
  int st = check_stream_args("rg_csr_compact_apply_columns_f32", a, &cg);
  if (st != RG_OK || n_vox == 0) return st;
  RG_REQUIRE(z_pieces >= 1 && z_pieces <= cg.n_planes, RG_EINVAL,
             "rg_csr_compact_apply_columns_f32: z_pieces=%d outside 1..planes=%ld", z_pieces, (long)cg.n_planes);
  RG_REQUIRE(!level_planes || (keep_lo >= 0 && n_keep >= 1 && keep_lo + (long)n_keep <= cg.n_planes), RG_EINVAL,
             "rg_csr_compact_apply_columns_f32: kept levels [%d, %d) outside the grid's %ld planes", keep_lo, keep_lo + n_keep,
             (long)cg.n_planes);
  RG_REQUIRE(!col_arg || col_max, RG_EINVAL, "rg_csr_compact_apply_columns_f32: col_arg needs col_max");
  RG_REQUIRE(!col_max || (col_lo >= 0 && col_lo <= col_hi && col_hi < cg.n_planes), RG_EINVAL,
             "rg_csr_compact_apply_columns_f32: column window [%d, %d] outside the grid's %ld planes", col_lo, col_hi,
             (long)cg.n_planes);
  const long n_xy = cg.lines_per_plane * cg.line_len;
  const long need_ws = (col_max && z_pieces > 1) ? (long)z_pieces * n_fields * n_xy * 8 : 0;
  RG_REQUIRE(need_ws == 0 || (workspace && workspace_bytes >= need_ws), RG_EWORKSPACE,
             "rg_csr_compact_apply_columns_f32: workspace of %ld bytes needed for %d level pieces (rg_csr_columns_workspace_bytes)",
             need_ws, z_pieces);
  const long n_cols = (long)cg.nyg * cg.nsx;
  RG_REQUIRE(n_cols * z_pieces <= 0x7FFFFFFFL, RG_EUNSUPPORTED, "rg_csr_compact_apply_columns_f32: too many workgroups");
  float* part_val = nullptr;
  int32_t* part_arg = nullptr;
  if (col_max && z_pieces > 1) {
    part_val = static_cast<float*>(workspace);
    part_arg = reinterpret_cast<int32_t*>(part_val + (size_t)z_pieces * n_fields * n_xy);
  }
  hipStream_t s = a.stream;
  {
    rgl::RowwiseColumns c;
    c.order = order;
    c.planes = level_planes;
    c.col_val = part_val ? part_val : col_max;
    c.col_arg = part_val ? part_arg : col_arg;
    c.n_xy = n_xy;
    c.n_cols = (unsigned)n_cols;
    c.pieces = z_pieces;
    c.keep_lo = level_planes ? keep_lo : 0;
    c.n_keep = level_planes ? n_keep : 0;
    c.col_lo = col_lo;
    c.col_hi = col_hi;
    st = launch_rowwise_cols(a, cg, c);
  }
  if (st != RG_OK) return st;
  if (part_val) {
    const long n = (long)n_fields * n_xy;
    hipLaunchKernelGGL(columns_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part_val, part_arg, z_pieces, n,
                       col_max, col_arg);
    return rg::check_launch("rg_csr_compact_apply_columns_f32 (merge)");
  }
  return RG_OK;
}

extern "C" int rg_csr_compact_apply_columns_f32(const void* indptr, int32_t indptr_is_i64, const void* records,
                                                const int64_t* rec_ptr, int32_t rec_order, uint32_t w_base,
                                                const int64_t* dict_ptr, const int32_t* dict, int64_t n_vox, int64_t n_pairs,
                                                int64_t line_len, int64_t lines_per_plane, const float* packed,
                                                int32_t n_fields, int32_t stride, int64_t n_gates, float fill_value,
                                                float* out, float* level_planes, int32_t keep_lo, int32_t n_keep,
                                                float* col_max, int32_t* col_arg, int32_t col_lo, int32_t col_hi,
                                                int32_t window_cap, int32_t z_pieces, const int32_t* order, void* workspace,
                                                int64_t workspace_bytes, int32_t lanes_hint, rg_stream_t stream) {
  return rg_csr_compact_apply_columns_f32_ex(indptr, indptr_is_i64, records, rec_ptr, rec_order, w_base, dict_ptr, dict, n_vox,
                                             n_pairs, line_len, lines_per_plane, packed, n_fields, stride, n_gates, fill_value,
                                             out, level_planes, keep_lo, n_keep, col_max, col_arg, col_lo, col_hi, window_cap,
                                             z_pieces, order, workspace, workspace_bytes, lanes_hint, nullptr, stream);
}

// K1q  rg_csr_compact_apply_planes_f32: the column mode with the wider epilogue (csr_compact_rowwise_kernel<..., PLANES = true>):
// COLMIN (radar_grid/products.py:493-535) and COLMEAN (:538-580) over the level window next to COLMAX, and the per-pixel
// levels of constant-elevation PPIs (:168-314) stored as samples for rg_elevation_ppi_finish_f32.  The min merges over level
// pieces like the max; the mean's float32 running sum cannot be split, so it takes one piece.
// Roofline: HBM.  As rg_csr_compact_apply_columns_f32, plus F*4*Vxy per min / mean plane, 4*Vxy per selection read and at most
// F*8*Vxy per selection written.
extern "C" int64_t rg_csr_planes_workspace_bytes(int64_t lines_per_plane, int64_t line_len, int32_t n_fields, int32_t z_pieces,
                                                 int32_t want_max, int32_t want_min) {
  if (lines_per_plane <= 0 || line_len <= 0 || n_fields < 1 || n_fields > 4 || z_pieces < 1) return RG_EINVAL;
  if (z_pieces == 1) return 0;
  return (int64_t)z_pieces * n_fields * lines_per_plane * line_len * ((want_max ? 8 : 0) + (want_min ? 4 : 0));
}

// _ex: with the row-end table of the grid (rg_csr_row_ends16; null = none, what rg_csr_compact_apply_planes_f32 passes)
extern "C" int rg_csr_compact_apply_planes_f32_ex(const void* indptr, int32_t indptr_is_i64, const void* records,
                                                  const int64_t* rec_ptr, int32_t rec_order, uint32_t w_base,
                                                  const int64_t* dict_ptr, const int32_t* dict, int64_t n_vox, int64_t n_pairs,
                                                  int64_t line_len, int64_t lines_per_plane, const float* packed,
                                                  int32_t n_fields, int32_t stride, int64_t n_gates, float fill_value,
                                                  const rg_plane_request* req, int32_t window_cap, int32_t z_pieces,
                                                  const int32_t* order, void* workspace, int64_t workspace_bytes,
                                                  int32_t lanes_hint, const uint16_t* row_end16, rg_stream_t stream) {
  RG_REQUIRE(req, RG_EINVAL, "rg_csr_compact_apply_planes_f32: null request");
  RG_REQUIRE(req->n_sel >= 0 && req->n_sel <= RG_MAX_SEL_PLANES, RG_EINVAL,
             "rg_csr_compact_apply_planes_f32: n_sel=%d outside 0..%d", req->n_sel, RG_MAX_SEL_PLANES);
  for (int k = 0; k < req->n_sel; ++k)
    RG_REQUIRE(req->sel_levels[k], RG_EINVAL, "rg_csr_compact_apply_planes_f32: sel_levels[%d] is null", k);
  RG_REQUIRE(req->n_sel == 0 || req->sel_samples, RG_EINVAL, "rg_csr_compact_apply_planes_f32: %d selections, null sel_samples",
             req->n_sel);
  RG_REQUIRE(req->out || req->level_planes || req->col_max || req->col_min || req->col_mean || req->n_sel > 0, RG_EINVAL,
             "rg_csr_compact_apply_planes_f32: nothing to produce");
  RG_REQUIRE(!(req->col_mean && z_pieces != 1), RG_EINVAL,
             "rg_csr_compact_apply_planes_f32: col_mean needs z_pieces == 1 (the float32 running sum cannot be split), got %d",
             z_pieces);
  RG_REQUIRE(!req->col_arg || req->col_max, RG_EINVAL, "rg_csr_compact_apply_planes_f32: col_arg needs col_max");
  const StreamArgs a{indptr, indptr_is_i64 != 0, records, rec_ptr, rec_order, w_base, dict_ptr, dict, n_vox, n_pairs, line_len,
                     lines_per_plane, packed, n_fields, stride, n_gates, fill_value, req->out, window_cap, lanes_hint,
                     (hipStream_t)stream, /*max_fields=*/4, /*need_out=*/false, /*need_packed=*/true, row_end16};
  ChunkGrid cg;
  int st = check_stream_args("rg_csr_compact_apply_planes_f32", a, &cg);
  if (st != RG_OK || n_vox == 0) return st;
  RG_REQUIRE(z_pieces >= 1 && z_pieces <= cg.n_planes, RG_EINVAL,
             "rg_csr_compact_apply_planes_f32: z_pieces=%d outside 1..planes=%ld", z_pieces, (long)cg.n_planes);
  RG_REQUIRE(req->n_sel == 0 || cg.n_planes < 0xFFFF, RG_EUNSUPPORTED,
             "rg_csr_compact_apply_planes_f32: level selections need fewer than 65535 planes, the grid has %ld", (long)cg.n_planes);
  RG_REQUIRE(!req->level_planes || (req->keep_lo >= 0 && req->n_keep >= 1 && req->keep_lo + (long)req->n_keep <= cg.n_planes),
             RG_EINVAL, "rg_csr_compact_apply_planes_f32: kept levels [%d, %d) outside the grid's %ld planes", req->keep_lo,
             req->keep_lo + req->n_keep, (long)cg.n_planes);
  const bool any_col = req->col_max || req->col_min || req->col_mean;
  RG_REQUIRE(!any_col || (req->col_lo >= 0 && req->col_lo <= req->col_hi && req->col_hi < cg.n_planes), RG_EINVAL,
             "rg_csr_compact_apply_planes_f32: column window [%d, %d] outside the grid's %ld planes", req->col_lo, req->col_hi,
             (long)cg.n_planes);
  const long n_xy = cg.lines_per_plane * cg.line_len;
  const bool split_max = req->col_max && z_pieces > 1, split_min = req->col_min && z_pieces > 1;
  const long need_ws = (long)z_pieces * n_fields * n_xy * ((split_max ? 8 : 0) + (split_min ? 4 : 0));
  RG_REQUIRE(need_ws == 0 || (workspace && workspace_bytes >= need_ws), RG_EWORKSPACE,
             "rg_csr_compact_apply_planes_f32: workspace of %ld bytes needed for %d level pieces (rg_csr_planes_workspace_bytes)",
             need_ws, z_pieces);
  const long n_cols = (long)cg.nyg * cg.nsx;
  RG_REQUIRE(n_cols * z_pieces <= 0x7FFFFFFFL, RG_EUNSUPPORTED, "rg_csr_compact_apply_planes_f32: too many workgroups");
  const size_t n_part = (size_t)z_pieces * n_fields * n_xy;
  float* part_val = split_max ? static_cast<float*>(workspace) : nullptr;
  int32_t* part_arg = split_max ? reinterpret_cast<int32_t*>(part_val + n_part) : nullptr;
  float* part_min = split_min ? static_cast<float*>(workspace) + (split_max ? 2 * n_part : 0) : nullptr;
  hipStream_t s = a.stream;
  {
    rgl::RowwisePlanes c;
    c.order = order;
    c.planes = req->level_planes;
    c.col_val = part_val ? part_val : req->col_max;
    c.col_arg = part_val ? part_arg : req->col_arg;
    c.n_xy = n_xy;
    c.n_cols = (unsigned)n_cols;
    c.pieces = z_pieces;
    c.keep_lo = req->level_planes ? req->keep_lo : 0;
    c.n_keep = req->level_planes ? req->n_keep : 0;
    c.col_lo = any_col ? req->col_lo : 0;
    c.col_hi = any_col ? req->col_hi : -1;
    c.col_min = part_min ? part_min : req->col_min;
    c.col_mean = req->col_mean;
    for (int k = 0; k < RG_MAX_SEL_PLANES; ++k) c.sel[k] = k < req->n_sel ? req->sel_levels[k] : nullptr;
    c.samples = req->n_sel ? req->sel_samples : nullptr;
    c.n_sel = req->n_sel;
    st = launch_rowwise_cols(a, cg, c);
  }
  if (st != RG_OK) return st;
  const long n = (long)n_fields * n_xy;
  const dim3 g((unsigned)((n + 255) / 256)), b(256);
  if (part_val) {
    hipLaunchKernelGGL(columns_merge_kernel, g, b, 0, s, part_val, part_arg, z_pieces, n, req->col_max, req->col_arg);
    st = rg::check_launch("rg_csr_compact_apply_planes_f32 (max merge)");
    if (st != RG_OK) return st;
  }
  if (part_min) {
    hipLaunchKernelGGL(planes_min_merge_kernel, g, b, 0, s, part_min, z_pieces, n, req->col_min);
    return rg::check_launch("rg_csr_compact_apply_planes_f32 (min merge)");
  }
  return RG_OK;
}

extern "C" int rg_csr_compact_apply_planes_f32(const void* indptr, int32_t indptr_is_i64, const void* records,
                                               const int64_t* rec_ptr, int32_t rec_order, uint32_t w_base,
                                               const int64_t* dict_ptr, const int32_t* dict, int64_t n_vox, int64_t n_pairs,
                                               int64_t line_len, int64_t lines_per_plane, const float* packed,
                                               int32_t n_fields, int32_t stride, int64_t n_gates, float fill_value,
                                               const rg_plane_request* req, int32_t window_cap, int32_t z_pieces,
                                               const int32_t* order, void* workspace, int64_t workspace_bytes,
                                               int32_t lanes_hint, rg_stream_t stream) {
  return rg_csr_compact_apply_planes_f32_ex(indptr, indptr_is_i64, records, rec_ptr, rec_order, w_base, dict_ptr, dict, n_vox,
                                            n_pairs, line_len, lines_per_plane, packed, n_fields, stride, n_gates, fill_value, req,
                                            window_cap, z_pieces, order, workspace, workspace_bytes, lanes_hint, nullptr, stream);
}
