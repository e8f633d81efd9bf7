// The grid mode of the row-wise kernel (rg_csr_rowwise.hpp) and the entry point rg_csr_compact_apply_packed_f32, which also
// reaches the tile kernel over the same records (rg_csr_compact.hip).
#include "rg_csr_rowwise.hpp"

namespace {

// Four fields, row sums in LDS instead of registers (one wavefront per SIMD more): taken when the window leaves room for five
// workgroups per CU next to the 8 KiB array.
constexpr long kLdsPerCu = 160 * 1024;
inline bool rowwise_lds_rowsums(int nf, int window_cap) {
  return nf == 4 && ((long)(window_cap + 1) * 4 * rowwise_entry_words<4>() + (long)kH * 64 * 4 * 8 + 512) * 5 <= kLdsPerCu;
}

// Grid mode, 1-8 fields: one workgroup per kRowwiseChunksPerBlock chunks of the dispatch order.
int launch_rowwise_grid(const StreamArgs& a, const ChunkGrid& cg) {
  constexpr int cpb = kRowwiseChunksPerBlock;
  const dim3 grid((unsigned)((chunk_count(cg) + cpb - 1) / cpb));
  const char* const fn = "rg_csr_compact_apply_packed_f32";
  return rg::dispatch_index(a.is_i64, [&](auto ind) {
    return rg::dispatch_fields(a.n_fields, [&](auto nf, auto) {
      using IndT = decltype(ind);
      constexpr int NF = decltype(nf)::value;
      const bool lds_sums = rowwise_lds_rowsums(NF, a.window_cap);
      const long static_lds = NF >= 5 ? (long)kH * 64 * 8 * 4 + 16                                     // the staged values of 5-8 fields
                                      : (RowwiseConfig<NF>::regs && !lds_sums) ? 16 : (long)kH * 64 * NF * 8;   // the row-sum array, if any
      if constexpr (NF == 4) {
        if (lds_sums) return launch_rowwise<IndT, NF, 0, 0>(fn, a, cg, static_lds, grid, cpb, RowwiseColumns());
      }
      return launch_rowwise<IndT, NF, 0, -1>(fn, a, cg, static_lds, grid, cpb, RowwiseColumns());
    });
  });
}

}  // namespace

// 1-4 fields over the packed stream.  tile = 0: the row-wise kernel (agrees with rg_csr_apply_f32 to float32 rounding);
// tile = 384: the tile kernel over the same records (agrees with it bit for bit);
// tile = 2000 + h: row-wise with a diagnostic lane split (h = 1..64: that many lanes per row; h = 70 + t: aim for t
// records per lane and row) -- a different split is a different order of the float32 adds.
// _ex: the same pass with the row-end table of the grid (rg_csr_row_ends16), which the row-wise kernel reads instead of the
// row pointers wherever a segment's span fits it; null = no table, which is what rg_csr_compact_apply_packed_f32 passes.
extern "C" int rg_csr_compact_apply_packed_f32_ex(const void* indptr, int32_t indptr_is_i64, const void* records,
                                                  const int64_t* rec_ptr, int32_t rec_order, uint32_t w_base,
                                                  const int64_t* dict_ptr,
                                                  const int32_t* dict, int64_t n_vox, int64_t n_pairs, int64_t line_len,
                                                  int64_t lines_per_plane, const float* packed, int32_t n_fields,
                                                  int32_t stride, int64_t n_gates, float fill_value, float* out,
                                                  int32_t window_cap, int32_t tile, const uint16_t* row_end16,
                                                  rg_stream_t stream) {
  const bool rowwise = tile == 0 || tile >= 2000;
  const int lanes_hint = tile >= 2000 ? tile - 2000 : 0;
  RG_REQUIRE(tile == 0 || tile == 384 ||
                 (tile >= 2000 && ((lanes_hint >= 1 && lanes_hint <= 64 && (lanes_hint & (lanes_hint - 1)) == 0) ||
                                   (lanes_hint > 70 && lanes_hint <= 99))),
             RG_EINVAL,
             "rg_csr_compact_apply_packed_f32: tile must be 0 (row-wise kernel), 384 (tile kernel) or 2000 + lane split");
  RG_REQUIRE(rowwise || n_fields <= 4, RG_EUNSUPPORTED,
             "rg_csr_compact_apply_packed_f32: n_fields=%d: the tile kernel over the records takes 1-4 fields (5-8 fields use "
             "128-pair tiles, not a whole number of 64-record loads); the row-wise kernel takes 1-8", n_fields);
  const StreamArgs a{indptr, indptr_is_i64 != 0, records, rec_ptr, rec_order, w_base, dict_ptr, dict, n_vox, n_pairs, line_len,
                     lines_per_plane, packed, n_fields, stride, n_gates, fill_value, out, window_cap, lanes_hint,
                     (hipStream_t)stream, /*max_fields=*/8, /*need_out=*/true, /*need_packed=*/false, row_end16};
  ChunkGrid cg;
  const int st = check_stream_args("rg_csr_compact_apply_packed_f32", a, &cg);
  if (st != RG_OK || n_vox == 0) return st;
  return rowwise ? launch_rowwise_grid(a, cg) : rg_launch_tile_packed(a, cg);
}

extern "C" int rg_csr_compact_apply_packed_f32(const void* indptr, int32_t indptr_is_i64, const void* records,
                                               const int64_t* rec_ptr, int32_t rec_order, uint32_t w_base,
                                               const int64_t* dict_ptr,
                                               const int32_t* dict, int64_t n_vox, int64_t n_pairs, int64_t line_len,
                                               int64_t lines_per_plane, const float* packed, int32_t n_fields,
                                               int32_t stride, int64_t n_gates, float fill_value, float* out,
                                               int32_t window_cap, int32_t tile, rg_stream_t stream) {
  return rg_csr_compact_apply_packed_f32_ex(indptr, indptr_is_i64, records, rec_ptr, rec_order, w_base, dict_ptr, dict, n_vox,
                                            n_pairs, line_len, lines_per_plane, packed, n_fields, stride, n_gates, fill_value,
                                            out, window_cap, tile, nullptr, stream);
}
