// The record packer of the compact CSR copy (layout: head of rg_csr_compact.hip; bit codings: rg_compact_layout.hpp):
// rg_csr_compact_pack_dense writes the packed pair stream that the row-wise kernel (rg_csr_rowwise.hpp) and the packed tile kernel read;
// rg_csr_compact_pack, its predecessor, is kept exported and refuses any work.
#include "rg_compact_layout.hpp"

// ---------------------------------------------------------------------------------------------------------------
// Packed pair stream: positions AND weights of three consecutive pairs of a segment in one record.
//   weight code = float32 bits of the weight minus w_base (= smallest exponent among the geometry's weights << 23); it
//   must fit 26 bits, i.e. all weights positive and within 8 binades -- Barnes weights span exp(-4)+1e-5 .. 1+1e-5, 7
//   binades; the host checks and falls back to the plain arrays otherwise.  Lossless: the kernel adds w_base back.
//   Two codings (bit layouts: rg_compact_layout.hpp), chosen per CHUNK from the size of its dictionary, which every reader
//   has at hand -- no flag travels with the records:
//     more than 2048 entries (the chunks at the radar, split chunks):  16 bytes, 16-bit positions, 5.33 bytes per pair
//     at most 2048 entries (99.9 % of the bench geometry's pairs):     14 bytes, 11-bit positions, 4.67 bytes per pair
//   The LOGICAL record is the same in both: record q of a segment holds its pairs 3q .. 3q + 2, so lanes, batch slots,
//   chains and the order of the adds do not know which coding they read.
//   Every segment (one wavefront's rows) starts on a 16-byte boundary; rec_ptr[slot] = its first 16-byte unit, and it takes
//   ceil(pairs / 3) units (wide) or ceil(14 * ceil(pairs / 3) / 16) (dense, the padding zeroed).  A dense record is read with
//   the aligned dwordx4 at (14 q) & ~3 -- its bytes start at byte 0 (q even) or 2 (q odd) of the load.
// ---------------------------------------------------------------------------------------------------------------
namespace {

template <typename IndT>
__global__ __launch_bounds__(256) void compact_pack_kernel(const IndT* __restrict__ indptr,
                                                            const uint16_t* __restrict__ lidx,
                                                            const float* __restrict__ wts, ChunkGrid cg, long n_slots,
                                                            int rec_order, const int64_t* __restrict__ dict_ptr,
                                                            const int64_t* __restrict__ rec_ptr,
                                                            unsigned w_base, rg_u32x4* __restrict__ rec,
                                                            int32_t* __restrict__ error_flag) {
  const int lane = threadIdx.x & 63;
  const long slot = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (slot >= n_slots) return;
  long r0;
  int nrows;
  unsigned chunk;
  if (rec_order == RG_REC_ORDER_DISPATCH) {      // slot = block * H + wavefront: the segment that wavefront reads
    const unsigned bid = (unsigned)(slot / kH);
    chunk = block_chunk(cg, bid);
    const Segment sg = chunk_segment(cg, chunk, (int)(slot - (long)bid * kH));
    r0 = sg.r0;
    nrows = sg.nrows;
  } else {                                       // slot = segment number, line-major
    const long line = slot / cg.nsx;
    const unsigned sx = (unsigned)(slot - line * cg.nsx);
    const unsigned x0 = sx * cg.seg_base + (sx < cg.seg_extra ? sx : cg.seg_extra);
    r0 = line * cg.line_len + x0;
    nrows = (int)(cg.seg_base + (sx < cg.seg_extra ? 1u : 0u));
    const long plane = line / cg.lines_per_plane;
    chunk = (unsigned)((plane * cg.nyg + (line - plane * cg.lines_per_plane) / kH) * cg.nsx + sx);
  }
  const bool dense = rec_is_dense(dict_ptr[chunk + 1] - dict_ptr[chunk]);     // the coding of this chunk's records
  const long p0 = nrows ? (long)indptr[r0] : 0, p1 = nrows ? (long)indptr[r0 + nrows] : 0;
  const long rn = (p1 - p0 + 2) / 3;             // records; rec_ptr counts 16-byte units
  const long rb = rec_ptr[slot], units = rec_ptr[slot + 1] - rb;
  if (lane == 0 && units != rec_units(rn, dense)) atomicOr(error_flag, 1);
  if (lane == 0 && rn >= (1L << 27)) atomicOr(error_flag, 4);   // the apply kernels use 32-bit byte offsets per segment
  if (units != rec_units(rn, dense)) return;     // never write outside the units rec_ptr gives this segment
  unsigned short* const half = reinterpret_cast<unsigned short*>(rec + rb);
  for (long r = lane; r < rn; r += 64) {
    unsigned code[3], pos[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const long p = p0 + 3 * r + j;
      code[j] = 0;
      pos[j] = 0;
      if (p < p1) {
        const unsigned bits = rg::f32_bits(wts[p]);
        code[j] = bits - w_base;
        if (bits < w_base || code[j] > 0x3FFFFFFu) atomicOr(error_flag, 2);   // not codable: the host checked, so never
        pos[j] = lidx[p];
        if (dense && pos[j] >= (unsigned)kDenseMaxDict) atomicOr(error_flag, 8);   // a position outside its dictionary
      }
    }
    if (dense) {
      unsigned short h[7];
      rec_encode_dense(code, pos, (r & 1) != 0, h);
#pragma unroll
      for (int j = 0; j < 7; ++j) half[7 * r + j] = h[j];
    } else {
      rg_u32x4 q;
      q.x = (code[0] & 0x3FFFFFFu) | ((pos[2] & 0x3Fu) << 26);
      q.y = (code[1] & 0x3FFFFFFu) | (((pos[2] >> 6) & 0x3Fu) << 26);
      q.z = (code[2] & 0x3FFFFFFu) | (((pos[2] >> 12) & 0xFu) << 26);
      q.w = pos[0] | (pos[1] << 16);
      rec[rb + r] = q;
    }
  }
  if (dense && 7 * rn + lane < 8 * units) half[7 * rn + lane] = 0;   // the padding up to the next unit (at most 7 halfwords)
}

}  // namespace

extern "C" int rg_csr_compact_pack_dense(const void* indptr, int32_t indptr_is_i64, const uint16_t* local_idx,
                                         const float* weights, int64_t n_rows, int64_t line_len, int64_t lines_per_plane,
                                         const int64_t* dict_ptr, const int64_t* rec_ptr, int32_t rec_order, int64_t plane0,
                                         uint32_t w_base, void* records, int32_t* error_flag, rg_stream_t stream) {
  RG_REQUIRE(n_rows >= 0 && plane0 >= 0, RG_EINVAL, "rg_csr_compact_pack_dense: negative size");
  RG_REQUIRE(rec_order == RG_REC_ORDER_SEGMENT || rec_order == RG_REC_ORDER_DISPATCH, RG_EINVAL,
             "rg_csr_compact_pack_dense: rec_order=%d is neither RG_REC_ORDER_SEGMENT nor RG_REC_ORDER_DISPATCH", rec_order);
  if (n_rows == 0) return RG_OK;
  RG_REQUIRE(indptr && dict_ptr && rec_ptr && error_flag, RG_EINVAL, "rg_csr_compact_pack_dense: null pointer");
  RG_REQUIRE(rg::aligned16(records), RG_EALIGN, "rg_csr_compact_pack_dense: records must be 16-byte aligned");
  ChunkGrid cg;
  RG_REQUIRE(make_chunk_grid(n_rows, line_len, lines_per_plane, &cg), RG_EINVAL,
             "rg_csr_compact_pack_dense: n_rows=%ld is not planes x lines_per_plane=%ld x line_len=%ld", (long)n_rows,
             (long)lines_per_plane, (long)line_len);
  RG_REQUIRE(chunk_count(cg) <= 0x7FFFFFFFL / kH, RG_EUNSUPPORTED, "rg_csr_compact_pack_dense: too many chunks for one launch");
  cg.grp0 = (unsigned)(((unsigned long)plane0 * cg.nyg) & 0xFFFFFFFFul);   // the rotation counts line groups mod 2^32
  const long n_slots = rec_order == RG_REC_ORDER_DISPATCH ? chunk_count(cg) * kH
                                                          : cg.n_planes * cg.lines_per_plane * (long)cg.nsx;
  const long blocks = (n_slots + 3) / 4;
  RG_REQUIRE(blocks <= 0x7FFFFFFFL, RG_EUNSUPPORTED, "rg_csr_compact_pack_dense: too many segments for one launch");
  hipStream_t s = (hipStream_t)stream;
  if (indptr_is_i64)
    hipLaunchKernelGGL(compact_pack_kernel<int64_t>, dim3((unsigned)blocks), dim3(256), 0, s,
                       static_cast<const int64_t*>(indptr), local_idx, weights, cg, n_slots, rec_order, dict_ptr, rec_ptr, w_base,
                       static_cast<rg_u32x4*>(records), error_flag);
  else
    hipLaunchKernelGGL(compact_pack_kernel<int32_t>, dim3((unsigned)blocks), dim3(256), 0, s,
                       static_cast<const int32_t*>(indptr), local_idx, weights, cg, n_slots, rec_order, dict_ptr, rec_ptr, w_base,
                       static_cast<rg_u32x4*>(records), error_flag);
  return rg::check_launch("rg_csr_compact_pack_dense");
}

// The packer of the 16-byte-only stream: it is given no dictionary sizes, so it cannot tell which chunks take the dense
// coding that every reader expects.  Kept exported with its signature; refuses any work.
extern "C" int rg_csr_compact_pack(const void* indptr, int32_t indptr_is_i64, const uint16_t* local_idx,
                                   const float* weights, int64_t n_rows, int64_t line_len, int64_t lines_per_plane,
                                   const int64_t* rec_ptr, int32_t rec_order, int64_t plane0, uint32_t w_base,
                                   void* records, int32_t* error_flag, rg_stream_t stream) {
  (void)indptr; (void)indptr_is_i64; (void)local_idx; (void)weights; (void)line_len; (void)lines_per_plane; (void)rec_ptr;
  (void)w_base; (void)records; (void)error_flag; (void)stream;
  RG_REQUIRE(n_rows >= 0 && plane0 >= 0, RG_EINVAL, "rg_csr_compact_pack: negative size");
  RG_REQUIRE(rec_order == RG_REC_ORDER_SEGMENT || rec_order == RG_REC_ORDER_DISPATCH, RG_EINVAL,
             "rg_csr_compact_pack: rec_order=%d is neither RG_REC_ORDER_SEGMENT nor RG_REC_ORDER_DISPATCH", rec_order);
  RG_REQUIRE(n_rows == 0, RG_EUNSUPPORTED,
             "rg_csr_compact_pack: the record coding depends on every chunk's dictionary size; call rg_csr_compact_pack_dense");
  return RG_OK;
}
