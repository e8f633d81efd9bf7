// K1c  csr_apply over a COMPACT device copy of the CSR.  Two families of kernels share the chunk layout, the
// dictionaries and the LDS field window described here:
//   * the TILE kernels (rg_csr_compact_apply_f32; rg_csr_compact_apply_packed_f32 with tile = 384), first half of this
//     file: rg_csr_apply_f32's pipeline minus its gather stage -- the same results as rg_csr_apply_f32, bit for bit;
//   * the ROW-WISE kernel (rg_csr_compact_apply_packed_f32, tile = 0; second half): no LDS tile at all, the default for
//     passes of 1-4 fields -- the same results to float32 rounding, in an order of its own.
//
// The reference's CSR (radar_grid/geometry.py:46-52) stores a 32-bit gate index per pair, and K1 pays for it twice:
// 4 of the 8 streamed bytes per pair, and one global gather per pair (F values wide), which the texture-address path
// serves at about 22 cycles per 64-lane instruction wherever the gates lie.  Neighbouring voxels share
// almost all their gates, so this copy groups the rows of a small 2-D PATCH of the grid into a chunk, lists the chunk's
// DISTINCT gates once (`dict`) and stores a 16-bit position in that list per pair:
//
//   chunk (plane z, line group yg, segment sx) = the segments sx of the H consecutive grid lines y = yg*H .. yg*H+H-1
//   of plane z; a segment = up to 64 consecutive rows of one line, exactly the unit one wavefront of rg_csr_apply_f32
//   owns.  A chunk therefore covers H x 64 voxels (H = RG_COMPACT_LINES = 4: 256 rows), a patch instead of a 256 x 1
//   strip: 2-3x fewer distinct gates per chunk, hence a smaller LDS window, more resident workgroups and fewer
//   dictionary bytes (measured per configuration in DESIGN.md);
//   bytes per pair 8 -> 6 (+ 4 bytes per distinct gate per chunk, 0.1-0.4 bytes per pair);
//   one workgroup = one chunk = H wavefronts: it gathers the chunk's few hundred field entries (F values each, the
//   rg_pack_fields_f32 layout) into an LDS window once -- coalesced reads of `dict`, one global gather per DISTINCT
//   gate -- and every pair then reads its values from LDS.  The window holds `window_cap` entries (chosen per geometry
//   to cover all but a handful of chunks -- those next to the radar, where every ray converges); a chunk with more
//   distinct gates gathers per pair through its dictionary instead.
//
// Tile kernels: pair order, weights, tiles and the float32 arithmetic are those of rg_csr_apply_f32 (same segments, same
// tiles, same products, same dynamic row phase), so they agree with it exactly for every field count.  The compact copy
// is derived from the standard CSR on the device (grid_geometry.CompactCSR) and the standard arrays stay the
// interchange format.
//
// Roofline: HBM.  Bytes per launch = 6*P + 4*D + sizeof(indptr)*(V+1) + 8*(C+1) + F*(5*G + 4*V)  with D = total
// dictionary entries, C = chunks; with the packed records (see rg_csr_compact_pack_dense) 16*U + 8*(S+1) replace 6*P, U = the
// 16-byte units the records take: ceil(14 n / 16) per segment of n records in a chunk of at most 2048 gates, n elsewhere.
#include "rg_compact_layout.hpp"

namespace {

// PACKED: positions and weights come from records of three pairs each (see rg_csr_compact_pack_dense: 14 or 16 bytes, by the
// chunk's dictionary size) instead of the 2-byte position and 4-byte weight arrays: 4.67 / 5.33 instead of 6 bytes per pair, one
// aligned dwordx4 per lane and 192 pairs.
template <typename IndT, int NF, int STRIDE, int TILE, bool PACKED = false>
__global__ __launch_bounds__(64 * kH) void csr_compact_kernel(
    const IndT* __restrict__ indptr, const uint16_t* __restrict__ lidx, const float* __restrict__ wts,
    const int64_t* __restrict__ dict_ptr, const int32_t* __restrict__ dict, ChunkGrid cg,
    const float* __restrict__ packed, unsigned last_gate, float fill, int window_cap, long n_vox,
    float* __restrict__ out, const rg_u32x4* __restrict__ rec, const int64_t* __restrict__ rec_ptr, unsigned w_base,
    int rec_order) {
  static_assert(TILE % 64 == 0, "a wave handles 64 pairs per step");
  static_assert(!PACKED || TILE % 192 == 0, "a packed tile is whole wave-loads of 64 three-pair records");
  constexpr int IT = TILE / 64;
  // window_cap entries: the packed slots of a gate (STRIDE floats), except that a 3-field entry drops the padding slot
  extern __shared__ __attribute__((aligned(16))) float window[];
  __shared__ __attribute__((aligned(16))) float tile_all[kH][TILE * rg::tile_floats(NF, STRIDE)];
  __shared__ f32x2 rowacc_all[kH][64 * NF];
  static_assert((sizeof(tile_all) + sizeof(rowacc_all)) % 16 == 0,
                "the dynamic window starts where the static arrays end and is accessed 16 bytes wide");
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* tile = tile_all[wv];
  f32x2* rowacc = rowacc_all[wv];

  const unsigned chunk = block_chunk(cg, blockIdx.x);
  const long d0 = dict_ptr[chunk];
  // A chunk's dictionary holds at most 65536 gates (positions are 16 bits).  The one exception is a SPLIT chunk -- more
  // distinct gates than that, as around the radar itself on a dense scan --, which stores one dictionary per wavefront
  // behind a header of kH offsets; its entry count (header included) exceeds 65536, which is how it is recognised.
  const int nd_all = (int)(dict_ptr[chunk + 1] - d0);
  const bool split = nd_all > 65536;
  const bool windowed = nd_all <= window_cap;        // workgroup-uniform; the rare wider chunk gathers per pair
  const int w_lo = split ? dict[d0 + wv] : 0;
  const int w_hi = split ? (wv + 1 < kH ? dict[d0 + wv + 1] : nd_all) : nd_all;
  const int nd = w_hi - w_lo;                        // entries of the dictionary this wavefront's positions refer to
  const int nd_last = nd > 0 ? nd - 1 : 0;
  const int32_t* __restrict__ cdict = dict + d0 + w_lo;

  const Segment sg = chunk_segment(cg, chunk, wv);
  const int nrows = sg.nrows;                        // wave-uniform; a wave without rows still helps to fill the window
  const long r0 = sg.r0;
  const long seg_b = nrows ? (long)indptr[r0] : 0;
  const long seg_e = nrows ? (long)indptr[r0 + nrows] : 0;
  const int span = (int)(seg_e - seg_b);
  const int rs_o = nrows ? (int)((long)indptr[r0 + (lane < nrows ? lane : nrows)] - seg_b) : 0;
  const int re_o = nrows ? (int)((long)indptr[r0 + (lane + 1 < nrows ? lane + 1 : nrows)] - seg_b) : 0;
#pragma unroll
  for (int f = 0; f < NF; ++f) rowacc[lane * NF + f] = (f32x2)(0.0f);

  // Two register stages, loop unrolled by two, every load unconditional and range-checked against the segment's last
  // pair -- the same exact-wait-count pipeline as rg_csr_apply_f32, without a gather stage.
  struct StagePlain {
    int ci[IT];
    float cw[IT];
  };
  struct StagePacked {
    rg_u32x4 r[PACKED ? IT / 3 : 1];
  };
  using Stage = std::conditional_t<PACKED, StagePacked, StagePlain>;
  Stage st[2];
  const uint16_t* __restrict__ li = lidx + seg_b;
  const float* __restrict__ wi = wts + seg_b;
  const int lane2 = lane * 2, lane4 = lane * 4;
  long rec_b = 0, rec_n = 0;                 // this segment's records (PACKED), in 16-byte units
  const bool dense = PACKED && rec_is_dense(nd_all);                        // 14-byte records (rg_compact_layout.hpp)
  const int rec_off = dense ? lane * 14 - (lane & 1) * 2 : lane * 16;       // the lane's aligned load within a wave-load
  if constexpr (PACKED) {
    if (nrows) {
      const long slot = rec_order == RG_REC_ORDER_DISPATCH ? (long)blockIdx.x * kH + wv : sg.seg;
      rec_b = rec_ptr[slot];
      rec_n = rec_ptr[slot + 1] - rec_b;
    }
  }
  auto stream = [&](Stage& sgs, int t) {   // t wave-uniform: the resources live in SGPRs
    if constexpr (PACKED) {
      const long r_t = t / 3;               // tiles are multiples of 192 pairs = 64 records: they start on an even record
      const long rbytes = r_t * (dense ? 14 : 16);
      const rsrc_t rr = make_rsrc(reinterpret_cast<const char*>(rec + rec_b) + rbytes, rec_n * 16 - rbytes);
      const int step = dense ? 64 * 14 : 1024;
#pragma unroll
      for (int k = 0; k < IT / 3; ++k) sgs.r[k] = rg_buffer_load_v4u32(rr, rec_off + k * step, 0, 0);
    } else {
      const rsrc_t ri = make_rsrc(li + t, ((long)span - t) * 2);
      const rsrc_t rw = make_rsrc(wi + t, ((long)span - t) * 4);
#pragma unroll
      for (int it = 0; it < IT; ++it) {
        sgs.ci[it] = (unsigned short)__builtin_amdgcn_raw_buffer_load_b16(ri, lane2 + it * 128, 0, 0);
        sgs.cw[it] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rw, lane4 + it * 256, 0, 0));
      }
    }
  };
  // pair slot `it` of a stage -> (position, weight) and its index in the tile.  Plain: pair it*64 + lane.  Packed: lane
  // holds record k = it / 3 of the tile's k-th wave-load, i.e. pairs k*192 + 3*lane + (it % 3); the record's coding
  // (16 bytes, or 14 in a chunk of at most 2048 gates) is rg_compact_layout.hpp's; w = float32 bits minus w_base.
  auto decode = [&](const Stage& sgs, int (&ci)[IT], float (&cw)[IT]) {
    if constexpr (PACKED) {
#pragma unroll
      for (int k = 0; k < IT / 3; ++k) {
        const RecFields f = dense ? rec_decode<true>(sgs.r[k], (unsigned)lane) : rec_decode<false>(sgs.r[k], 0u);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          cw[3 * k + j] = __builtin_bit_cast(float, (f.wc[j] & 0x3FFFFFFu) + w_base);
          ci[3 * k + j] = (int)f.pos[j];
        }
      }
    } else {
#pragma unroll
      for (int it = 0; it < IT; ++it) {
        ci[it] = sgs.ci[it];
        cw[it] = sgs.cw[it];
      }
    }
  };
  auto eidx = [&](int it) -> int { return PACKED ? (it / 3) * 192 + 3 * lane + (it % 3) : it * 64 + lane; };
  // the first two tiles are requested BEFORE the window is filled: the two latencies overlap
  stream(st[0], 0);
  stream(st[1], TILE);

  // ---- the chunk's field window: one gather per DISTINCT gate --------------------------------------------
  if (windowed) {
    for (int i = threadIdx.x; i < nd_all; i += 64 * kH) {
      const unsigned g0 = (unsigned)cdict[i];
      const unsigned g = g0 < last_gate ? g0 : last_gate;   // clamp: never fault
      float v[STRIDE];
      rg::load_packed<STRIDE>(packed, g, v);
      if constexpr (STRIDE == 1) {
        window[i] = v[0];
      } else if constexpr (STRIDE == 2) {
        reinterpret_cast<f32x2*>(window)[i] = (f32x2){v[0], v[1]};
      } else if constexpr (NF == 3) {
        window[i * 3] = v[0]; window[i * 3 + 1] = v[1]; window[i * 3 + 2] = v[2];
      } else {
#pragma unroll
        for (int q = 0; q < STRIDE; q += 4)
          reinterpret_cast<f32x4*>(window)[(size_t)i * (STRIDE / 4) + q / 4] = (f32x4){v[q], v[q + 1], v[q + 2], v[q + 3]};
      }
    }
  }
  __syncthreads();

  // The tile loop exists twice -- values from the LDS window, or (over-wide chunk) position -> gate -> value from memory
  // -- selected once per workgroup: a uniform branch INSIDE the unrolled loads made this compiler drop the register
  // copies of the last windowed read of a tile (3-field kernel, seen in the ISA), and the loop is leaner without it.
  auto run = [&](auto wtag) {
    constexpr bool kWindowed = decltype(wtag)::value;
    auto step = [&](int t, Stage& cur) {
      // ---- values of tile t ---------------------------------------------------------------------------------
      float val[IT][STRIDE];
      int ci[IT];
      float cw[IT];
      decode(cur, ci, cw);
#pragma unroll
      for (int it = 0; it < IT; ++it) {
        const int pos = ci[it] < nd_last ? ci[it] : nd_last;
        if constexpr (kWindowed) {
          if constexpr (STRIDE == 1) {
            val[it][0] = window[pos];
          } else if constexpr (STRIDE == 2) {
            const f32x2 q = reinterpret_cast<const f32x2*>(window)[pos];
            val[it][0] = q.x; val[it][1] = q.y;
          } else if constexpr (NF == 3) {
            val[it][0] = window[pos * 3]; val[it][1] = window[pos * 3 + 1]; val[it][2] = window[pos * 3 + 2];
            val[it][3] = 0.0f;   // the padding slot is never looked at
          } else {
#pragma unroll
            for (int s = 0; s < STRIDE; s += 4) {
              const f32x4 q = reinterpret_cast<const f32x4*>(window)[(size_t)pos * (STRIDE / 4) + s / 4];
              val[it][s] = q.x; val[it][s + 1] = q.y; val[it][s + 2] = q.z; val[it][s + 3] = q.w;
            }
          }
        } else {
          const unsigned g0 = (unsigned)cdict[pos];
          const unsigned gc = g0 < last_gate ? g0 : last_gate;
          rg::load_packed<STRIDE>(packed, gc, val[it]);
        }
      }
      // ---- products of tile t -> LDS (layout and arithmetic: rg_row_phase.hpp) ----------------------------------
#pragma unroll
      for (int it = 0; it < IT; ++it) rg::store_products<NF, STRIDE>(tile, TILE, eidx(it), cw[it], val[it]);
      stream(cur, t + 2 * TILE);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

      // ---- dynamic row phase (shared with rg_csr_apply_f32: same lane split, same float32 adds) ----------------
      rg::row_phase<NF, STRIDE, TILE>(tile, rowacc, t, rs_o, re_o, lane);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };

    for (int t = 0; t < span;) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        step(t, st[u]);
        t += TILE;
        if (t >= span) break;
      }
    }
  };
  if (span > 0) {
    if (windowed) run(std::true_type{}); else run(std::false_type{});
  }

  if (lane < nrows) {
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const f32x2 s = rowacc[lane * NF + f];
      out[(size_t)f * n_vox + r0 + lane] = s.y > 0.0f ? (float)((double)s.x / (double)s.y) : fill;
    }
  }
}


template <typename IndT, int NF, int TILE>
constexpr size_t static_lds() {
  return (size_t)kH * (TILE * rg::tile_floats(NF, stride_for(NF)) * 4 + 64 * NF * 8);
}

struct PackedStream {   // the packed form of positions + weights (rg_csr_compact_pack); null = the plain arrays
  const rg_u32x4* rec = nullptr;
  const int64_t* rec_ptr = nullptr;
  unsigned w_base = 0;
  int order = RG_REC_ORDER_SEGMENT;
};

template <typename IndT, int NF, int TILE, bool PACKED = false>
int launch_nf(int window_cap, const void* indptr, const uint16_t* lidx, const float* wts, const int64_t* dict_ptr,
              const int32_t* dict, const ChunkGrid& cg, long n_vox, const float* packed, long n_gates, float fill,
              float* out, hipStream_t s, PackedStream ps = PackedStream()) {
  constexpr int STRIDE = stride_for(NF);
  // static + dynamic LDS of one workgroup stay within the 64 KiB a launch gets without opting in to more; a window
  // smaller than the geometry asked for only sends more chunks down the per-pair path (same results)
  constexpr int WS = NF == 3 ? 3 : STRIDE;   // floats per window entry (see the kernel)
  const long room = (65536 - (long)static_lds<IndT, NF, TILE>() - 256) / (4 * WS);
  if (window_cap > room) window_cap = (int)(room < 0 ? 0 : room);
  hipLaunchKernelGGL((csr_compact_kernel<IndT, NF, STRIDE, TILE, PACKED>), dim3((unsigned)chunk_count(cg)),
                     dim3(64 * kH), ((size_t)window_cap * WS * sizeof(float) + 15) / 16 * 16, s,
                     static_cast<const IndT*>(indptr), lidx, wts, dict_ptr, dict, cg, packed, (unsigned)(n_gates - 1), fill,
                     window_cap, n_vox, out, ps.rec, ps.rec_ptr, ps.w_base, ps.order);
  return rg::check_launch("rg_csr_compact_apply_f32");
}

// Tiles: the defaults MUST be the tiles rg_csr_apply_f32 uses for the same field count (same partial sums).
template <typename IndT>
int launch(int nf, int tile, int window_cap, const void* indptr, const uint16_t* lidx, const float* wts,
           const int64_t* dict_ptr, const int32_t* dict, const ChunkGrid& cg, long n_vox, const float* packed, long n_gates,
           float fill, float* out, hipStream_t s) {
#define RG_K1C(NF_, TILE_) \
  launch_nf<IndT, NF_, TILE_>(window_cap, indptr, lidx, wts, dict_ptr, dict, cg, n_vox, packed, n_gates, fill, out, s)
  switch (nf) {
    case 1:
      switch (tile) {
        case 128: return RG_K1C(1, 128);
        case 256: return RG_K1C(1, 256);
        case 512: return RG_K1C(1, 512);
        default: return RG_K1C(1, 384);
      }
    case 2:
      switch (tile) {
        case 128: return RG_K1C(2, 128);
        case 256: return RG_K1C(2, 256);
        case 512: return RG_K1C(2, 512);
        default: return RG_K1C(2, 384);
      }
    case 3:
      switch (tile) {
        case 128: return RG_K1C(3, 128);
        case 192: return RG_K1C(3, 192);
        case 256: return RG_K1C(3, 256);
        case 320: return RG_K1C(3, 320);
        default: return RG_K1C(3, 384);
      }
    case 4:
      switch (tile) {
        case 128: return RG_K1C(4, 128);
        case 256: return RG_K1C(4, 256);
        case 320: return RG_K1C(4, 320);
        default: return RG_K1C(4, 384);
      }
    case 5: return RG_K1C(5, 128);
    case 6: return RG_K1C(6, 128);
    case 7: return RG_K1C(7, 128);
    default: return RG_K1C(8, 128);
  }
#undef RG_K1C
}

}  // namespace

extern "C" int64_t rg_csr_compact_chunks(int64_t n_rows, int64_t line_len, int64_t lines_per_plane) {
  ChunkGrid cg;
  if (n_rows < 0 || !make_chunk_grid(n_rows, line_len, lines_per_plane, &cg)) return RG_EINVAL;
  return n_rows == 0 ? 0 : chunk_count(cg);
}

extern "C" int rg_csr_compact_apply_f32(const void* indptr, int32_t indptr_is_i64, const uint16_t* local_idx,
                                        const float* weights, const int64_t* dict_ptr, const int32_t* dict,
                                        int64_t n_vox, int64_t n_pairs, int64_t line_len, int64_t lines_per_plane,
                                        const float* packed, int32_t n_fields, int32_t stride, int64_t n_gates,
                                        float fill_value, float* out, int32_t window_cap, int32_t tile,
                                        rg_stream_t stream) {
  RG_REQUIRE(indptr && out && dict_ptr, RG_EINVAL, "rg_csr_compact_apply_f32: null indptr/dict_ptr/out");
  RG_REQUIRE(n_vox >= 0 && n_pairs >= 0, RG_EINVAL, "rg_csr_compact_apply_f32: negative size");
  RG_REQUIRE(n_fields >= 1 && n_fields <= RG_MAX_FIELDS, RG_EUNSUPPORTED,
             "rg_csr_compact_apply_f32: n_fields=%d not in 1..%d", n_fields, RG_MAX_FIELDS);
  RG_REQUIRE(stride == stride_for(n_fields), RG_EINVAL, "rg_csr_compact_apply_f32: stride=%d, expected %d for %d fields",
             stride, stride_for(n_fields), n_fields);
  RG_REQUIRE(n_pairs == 0 || (local_idx && weights && dict && packed && n_gates > 0), RG_EINVAL,
             "rg_csr_compact_apply_f32: pairs present but local_idx/weights/dict/packed/n_gates missing");
  RG_REQUIRE(n_gates <= 0x7FFFFFFFL, RG_EUNSUPPORTED, "rg_csr_compact_apply_f32: n_gates exceeds int32 gate indices");
  RG_REQUIRE(n_vox <= 0x3FFFFFFFFFL, RG_EUNSUPPORTED, "rg_csr_compact_apply_f32: n_vox too large for one launch");
  RG_REQUIRE(tile == 0 || tile == 128 || tile == 192 || tile == 256 || tile == 320 || tile == 384 || tile == 512,
             RG_EINVAL, "rg_csr_compact_apply_f32: tile must be 0 (default), 128, 192, 256, 320, 384 or 512");
  RG_REQUIRE(window_cap >= 0 && window_cap <= RG_COMPACT_MAX_WINDOW, RG_EINVAL,
             "rg_csr_compact_apply_f32: window_cap %d outside 0..%d", window_cap, RG_COMPACT_MAX_WINDOW);
  RG_REQUIRE(rg::aligned16(packed), RG_EALIGN, "rg_csr_compact_apply_f32: packed must be 16-byte aligned");
  if (n_vox == 0) return RG_OK;
  ChunkGrid cg;
  RG_REQUIRE(make_chunk_grid(n_vox, line_len, lines_per_plane, &cg), RG_EINVAL,
             "rg_csr_compact_apply_f32: n_vox=%ld is not planes x lines_per_plane=%ld x line_len=%ld", (long)n_vox,
             (long)lines_per_plane, (long)line_len);
  RG_REQUIRE(chunk_count(cg) <= 0x7FFFFFFFL, RG_EUNSUPPORTED, "rg_csr_compact_apply_f32: too many chunks for one launch");
  hipStream_t s = (hipStream_t)stream;
  if (indptr_is_i64)
    return launch<int64_t>(n_fields, tile, window_cap, indptr, local_idx, weights, dict_ptr, dict, cg, n_vox, packed,
                           n_gates, fill_value, out, s);
  return launch<int32_t>(n_fields, tile, window_cap, indptr, local_idx, weights, dict_ptr, dict, cg, n_vox, packed, n_gates,
                         fill_value, out, s);
}

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

// ---------------------------------------------------------------------------------------------------------------
// Row-wise kernel over the packed stream (1-4 fields): the default of rg_csr_compact_apply_packed_f32.
// The tile kernel above moves every pair through LDS twice (the product side writes the tile, the row side reads it
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
// constraint, which is what the row-wise kernel itself measured best with.  COLS == 2 (planes mode): the wider epilogue is
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
    int rec_order, unsigned n_chunks, int chunks_per_block, const std::conditional_t<COLS == 2, RowwisePlanes, RowwiseColumns> cols) {
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
  for (int cb = 0; cb < chunks_per_block; ++cb) {
  unsigned bid, chunk;
  if constexpr (COLS) {
    const unsigned grp = (unsigned)(col_z0 + cb) * cg.nyg + col_yg;
    chunk = grp * cg.nsx + col_sx;
    const unsigned shift = ((grp + cg.grp0) * cg.rot_step) % cg.nsx;      // the block whose rotated column is col_sx
    bid = grp * cg.nsx + (col_sx >= shift ? col_sx - shift : col_sx + cg.nsx - shift);
  } else {
    bid = blockIdx.x * (unsigned)chunks_per_block + (unsigned)cb;
    if (bid >= n_chunks) break;                       // workgroup-uniform
    chunk = block_chunk(cg, bid);
  }
  if (cb > 0) __syncthreads();                        // every wavefront is done with the previous chunk's window
  float mine_p[NF], mine_w[NF];                       // kRegs: lane == row
#pragma unroll
  for (int f = 0; f < NF; ++f) mine_p[f] = mine_w[f] = 0.0f;

  const long d0 = dict_ptr[chunk];
  const int nd_all = (int)(dict_ptr[chunk + 1] - d0);
  const bool split = nd_all > 65536;
  const bool windowed = nd_all <= window_cap;        // the window holds window_cap + 1 entries: the sentinel
  const int w_lo = split ? dict[d0 + wv] : 0;
  const int w_hi = split ? (wv + 1 < kH ? dict[d0 + wv + 1] : nd_all) : nd_all;
  const int nd = w_hi - w_lo;
  const int nd_last = nd > 0 ? nd - 1 : 0;
  const int32_t* __restrict__ cdict = dict + d0 + w_lo;

  const Segment sg = chunk_segment(cg, chunk, wv);
  const int nrows = sg.nrows;
  const long r0 = sg.r0;
  const long seg_b = nrows ? (long)indptr[r0] : 0;
  const long seg_e = nrows ? (long)indptr[r0 + nrows] : 0;
  const int span = (int)(seg_e - seg_b);
  const int rs_o = nrows ? (int)((long)indptr[r0 + (lane < nrows ? lane : nrows)] - seg_b) : 0;
  const int re_o = nrows ? (int)((long)indptr[r0 + (lane + 1 < nrows ? lane + 1 : nrows)] - seg_b) : 0;
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
    const int32_t* __restrict__ cd = nd_all > 0 ? cdict : (const int32_t*)dict_ptr;   // never dereference an empty dictionary
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
      // the record's pairs i = 0, 1, 2 belong to the lane's row iff lo <= i < lo + len (len = 0 for a lane without record)
      const int lo = r.lo0 - 3 * (k << lgl);
      const unsigned len = (kDense ? 2 * (k << lgl) + 1 < r.rem : (k << lgl) < r.rem) ? r.len : 0u;
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
        const bool mine = (unsigned)(i - lo) < len;
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
      const f32x4 lo = reinterpret_cast<const f32x4*>(stage)[2 * lane], hi = reinterpret_cast<const f32x4*>(stage)[2 * lane + 1];
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

// Four fields, row sums in LDS instead of registers (one wavefront per SIMD more): taken when the window leaves room for five
// workgroups per CU next to the 8 KiB array.
constexpr long kLdsPerCu = 160 * 1024;
inline bool rowwise_lds_rowsums(int nf, int window_cap) {
  return nf == 4 && ((long)(window_cap + 1) * 4 * rowwise_entry_words<4>() + (long)kH * 64 * 4 * 8 + 512) * 5 <= kLdsPerCu;
}

template <typename IndT, int NF>
int launch_rowwise(int window_cap, const void* indptr, const int64_t* dict_ptr, const int32_t* dict, const ChunkGrid& cg,
                   long n_vox, const float* packed, long n_gates, float fill, float* out, hipStream_t s,
                   const PackedStream& ps, int lanes_hint) {
  constexpr int STRIDE = stride_for(NF);
  constexpr int WS = rowwise_entry_words<NF>();                                   // 4-byte words per window entry
  const bool lds_sums = rowwise_lds_rowsums(NF, window_cap);
  const long kStatic = NF >= 5 ? (long)kH * 64 * 8 * 4 + 16                                     // the staged values of 5-8 fields
                               : (RowwiseConfig<NF>::regs && !lds_sums) ? 16 : (long)kH * 64 * NF * 8;   // the row-sum array, if any
  // one entry beyond window_cap: the sentinel; a smaller window only sends more chunks down the per-pair path
  const long room = (65536 - kStatic - 256) / (4 * WS) - 1;
  if (window_cap > room) window_cap = (int)room;
  const long n_chunks = chunk_count(cg);
  constexpr int cpb = kRowwiseChunksPerBlock;
  const dim3 grid((unsigned)((n_chunks + cpb - 1) / cpb)), block(64 * kH);
  const size_t lds = ((size_t)(window_cap + 1) * WS * sizeof(float) + 15) / 16 * 16;
#define RG_ROWWISE_LAUNCH(REGS_)                                                                                              \
  hipLaunchKernelGGL((csr_compact_rowwise_kernel<IndT, NF, STRIDE, 0, REGS_>), grid, block, lds, s,                        \
                     static_cast<const IndT*>(indptr), dict_ptr, dict, cg, packed, (unsigned)(n_gates - 1), fill, window_cap, \
                     n_vox, out, ps.rec, ps.rec_ptr, ps.w_base, lanes_hint, ps.order, (unsigned)n_chunks, cpb,                \
                     RowwiseColumns())
  if constexpr (NF == 4) {
    if (lds_sums) RG_ROWWISE_LAUNCH(0); else RG_ROWWISE_LAUNCH(-1);
  } else {
    RG_ROWWISE_LAUNCH(-1);
  }
#undef RG_ROWWISE_LAUNCH
  return rg::check_launch("rg_csr_compact_apply_packed_f32");
}

}  // namespace

// Column mode of the row-wise kernel: the launcher rg_csr_columns.hip calls (declared in rg_compact_layout.hpp).
template <typename IndT, int NF, bool PLANES = false, typename Cols = RowwiseColumns>
static int launch_rowwise_columns_t(int window_cap, const void* indptr, const int64_t* dict_ptr, const int32_t* dict,
                                    const ChunkGrid& cg, long n_vox, const float* packed, long n_gates, float fill, float* out,
                                    hipStream_t s, const void* rec, const int64_t* rec_ptr, unsigned w_base, int rec_order,
                                    int lanes_hint, const Cols& cols) {
  constexpr int STRIDE = stride_for(NF);
  constexpr int WS = rowwise_entry_words<NF>();
  constexpr int kRegsCols = -1;      // (four fields with the row sums in LDS: 108 instead of 111 VGPRs, the same 4 wavefronts)
  constexpr long kStatic = RowwiseConfig<NF>::regs ? 16 : (long)kH * 64 * NF * 8;
  const long room = (65536 - kStatic - 256) / (4 * WS) - 1;
  if (window_cap > room) window_cap = (int)room;
  hipLaunchKernelGGL((csr_compact_rowwise_kernel<IndT, NF, STRIDE, PLANES ? 2 : 1, kRegsCols>), dim3(cols.n_cols * (unsigned)cols.pieces),
                     dim3(64 * kH), ((size_t)(window_cap + 1) * WS * sizeof(float) + 15) / 16 * 16, s,
                     static_cast<const IndT*>(indptr), dict_ptr, dict, cg, packed, (unsigned)(n_gates - 1), fill, window_cap, n_vox,
                     out, static_cast<const rg_u32x4*>(rec), rec_ptr, w_base, lanes_hint, rec_order,
                     (unsigned)chunk_count(cg), 1, cols);
  return rg::check_launch(PLANES ? "rg_csr_compact_apply_planes_f32" : "rg_csr_compact_apply_columns_f32");
}

int rg_launch_rowwise_columns(int nf, bool i64, int window_cap, const void* indptr, const int64_t* dict_ptr, const int32_t* dict,
                              const ChunkGrid& cg, long n_vox, const float* packed, long n_gates, float fill, float* out,
                              hipStream_t s, const void* rec, const int64_t* rec_ptr, unsigned w_base, int rec_order,
                              int lanes_hint, const RowwiseColumns& cols) {
#define RG_COLS(IND_, NF_) \
  launch_rowwise_columns_t<IND_, NF_>(window_cap, indptr, dict_ptr, dict, cg, n_vox, packed, n_gates, fill, out, s, rec, rec_ptr, \
                                      w_base, rec_order, lanes_hint, cols)
  if (i64) {
    switch (nf) {
      case 1: return RG_COLS(int64_t, 1);
      case 2: return RG_COLS(int64_t, 2);
      case 3: return RG_COLS(int64_t, 3);
      default: return RG_COLS(int64_t, 4);
    }
  }
  switch (nf) {
    case 1: return RG_COLS(int32_t, 1);
    case 2: return RG_COLS(int32_t, 2);
    case 3: return RG_COLS(int32_t, 3);
    default: return RG_COLS(int32_t, 4);
  }
#undef RG_COLS
}

// Planes mode (rg_csr_compact_apply_planes_f32): the same launch with the wider epilogue.
int rg_launch_rowwise_planes(int nf, bool i64, int window_cap, const void* indptr, const int64_t* dict_ptr, const int32_t* dict,
                             const ChunkGrid& cg, long n_vox, const float* packed, long n_gates, float fill, float* out,
                             hipStream_t s, const void* rec, const int64_t* rec_ptr, unsigned w_base, int rec_order,
                             int lanes_hint, const RowwisePlanes& cols) {
#define RG_PLANES(IND_, NF_) \
  launch_rowwise_columns_t<IND_, NF_, true>(window_cap, indptr, dict_ptr, dict, cg, n_vox, packed, n_gates, fill, out, s, rec,  \
                                            rec_ptr, w_base, rec_order, lanes_hint, cols)
  if (i64) {
    switch (nf) {
      case 1: return RG_PLANES(int64_t, 1);
      case 2: return RG_PLANES(int64_t, 2);
      case 3: return RG_PLANES(int64_t, 3);
      default: return RG_PLANES(int64_t, 4);
    }
  }
  switch (nf) {
    case 1: return RG_PLANES(int32_t, 1);
    case 2: return RG_PLANES(int32_t, 2);
    case 3: return RG_PLANES(int32_t, 3);
    default: return RG_PLANES(int32_t, 4);
  }
#undef RG_PLANES
}

namespace {

template <typename IndT>
int launch_rowwise_nf(int nf, int window_cap, const void* indptr, const int64_t* dict_ptr, const int32_t* dict,
                      const ChunkGrid& cg, long n_vox, const float* packed, long n_gates, float fill, float* out,
                      hipStream_t s, const PackedStream& ps, int lanes_hint) {
#define RG_ROW(NF_) \
  launch_rowwise<IndT, NF_>(window_cap, indptr, dict_ptr, dict, cg, n_vox, packed, n_gates, fill, out, s, ps, lanes_hint)
  switch (nf) {
    case 1: return RG_ROW(1);
    case 2: return RG_ROW(2);
    case 3: return RG_ROW(3);
    case 4: return RG_ROW(4);
    case 5: return RG_ROW(5);
    case 6: return RG_ROW(6);
    case 7: return RG_ROW(7);
    default: return RG_ROW(8);
  }
#undef RG_ROW
}

}  // namespace

// 1-4 fields over the packed stream.  tile = 0: the row-wise kernel (agrees with rg_csr_apply_f32 to float32 rounding);
// tile = 384: the tile kernel over the same records (agrees with it bit for bit);
// tile = 2000 + h: row-wise with a diagnostic lane split (h = 1..64: that many lanes per row; h = 70 + t: aim for t
// records per lane and row) -- a different split is a different order of the float32 adds.
extern "C" int rg_csr_compact_apply_packed_f32(const void* indptr, int32_t indptr_is_i64, const void* records,
                                               const int64_t* rec_ptr, int32_t rec_order, uint32_t w_base,
                                               const int64_t* dict_ptr,
                                               const int32_t* dict, int64_t n_vox, int64_t n_pairs, int64_t line_len,
                                               int64_t lines_per_plane, const float* packed, int32_t n_fields,
                                               int32_t stride, int64_t n_gates, float fill_value, float* out,
                                               int32_t window_cap, int32_t tile, rg_stream_t stream) {
  const bool rowwise = tile == 0 || tile >= 2000;
  const int lanes_hint = tile >= 2000 ? tile - 2000 : 0;
  RG_REQUIRE(tile == 0 || tile == 384 ||
                 (tile >= 2000 && ((lanes_hint >= 1 && lanes_hint <= 64 && (lanes_hint & (lanes_hint - 1)) == 0) ||
                                   (lanes_hint > 70 && lanes_hint <= 99))),
             RG_EINVAL,
             "rg_csr_compact_apply_packed_f32: tile must be 0 (row-wise kernel), 384 (tile kernel) or 2000 + lane split");
  RG_REQUIRE(rec_order == RG_REC_ORDER_SEGMENT || rec_order == RG_REC_ORDER_DISPATCH, RG_EINVAL,
             "rg_csr_compact_apply_packed_f32: rec_order=%d is neither RG_REC_ORDER_SEGMENT nor RG_REC_ORDER_DISPATCH", rec_order);
  RG_REQUIRE(n_fields >= 1 && n_fields <= (rowwise ? 8 : 4), RG_EUNSUPPORTED,
             "rg_csr_compact_apply_packed_f32: n_fields=%d not in 1..%d (the row-wise kernel takes 1-8 fields; the tile kernel "
             "over the records 1-4: 5-8 fields use 128-pair tiles, not a whole number of 64-record loads)", n_fields,
             rowwise ? 8 : 4);
  RG_REQUIRE(stride == stride_for(n_fields), RG_EINVAL, "rg_csr_compact_apply_packed_f32: stride=%d, expected %d for %d fields",
             stride, stride_for(n_fields), n_fields);
  RG_REQUIRE(indptr && out && dict_ptr && rec_ptr, RG_EINVAL, "rg_csr_compact_apply_packed_f32: null indptr/dict_ptr/rec_ptr/out");
  RG_REQUIRE(n_vox >= 0 && n_pairs >= 0, RG_EINVAL, "rg_csr_compact_apply_packed_f32: negative size");
  RG_REQUIRE(n_pairs == 0 || (records && dict && packed && n_gates > 0), RG_EINVAL,
             "rg_csr_compact_apply_packed_f32: pairs present but records/dict/packed/n_gates missing");
  RG_REQUIRE(n_gates <= 0x7FFFFFFFL, RG_EUNSUPPORTED, "rg_csr_compact_apply_packed_f32: n_gates exceeds int32 gate indices");
  RG_REQUIRE(n_vox <= 0x3FFFFFFFFFL, RG_EUNSUPPORTED, "rg_csr_compact_apply_packed_f32: n_vox too large for one launch");
  RG_REQUIRE(window_cap >= 0 && window_cap <= RG_COMPACT_MAX_WINDOW, RG_EINVAL,
             "rg_csr_compact_apply_packed_f32: window_cap %d outside 0..%d", window_cap, RG_COMPACT_MAX_WINDOW);
  RG_REQUIRE(rg::aligned16(records), RG_EALIGN, "rg_csr_compact_apply_packed_f32: records must be 16-byte aligned");
  RG_REQUIRE((w_base & 0x3FFFFFFu) == 0, RG_EINVAL,
             "rg_csr_compact_apply_packed_f32: w_base=0x%08x must have its low 26 bits clear (exponent a multiple of 8)", w_base);
  if (n_vox == 0) return RG_OK;
  ChunkGrid cg;
  RG_REQUIRE(make_chunk_grid(n_vox, line_len, lines_per_plane, &cg), RG_EINVAL,
             "rg_csr_compact_apply_packed_f32: n_vox=%ld is not planes x lines_per_plane=%ld x line_len=%ld", (long)n_vox,
             (long)lines_per_plane, (long)line_len);
  RG_REQUIRE(chunk_count(cg) <= 0x7FFFFFFFL, RG_EUNSUPPORTED, "rg_csr_compact_apply_packed_f32: too many chunks for one launch");
  PackedStream ps;
  ps.rec = static_cast<const rg_u32x4*>(records);
  ps.rec_ptr = rec_ptr;
  ps.w_base = w_base;
  ps.order = rec_order;
  hipStream_t s = (hipStream_t)stream;
  if (rowwise)
    return indptr_is_i64 ? launch_rowwise_nf<int64_t>(n_fields, window_cap, indptr, dict_ptr, dict, cg, n_vox, packed, n_gates,
                                                      fill_value, out, s, ps, lanes_hint)
                         : launch_rowwise_nf<int32_t>(n_fields, window_cap, indptr, dict_ptr, dict, cg, n_vox, packed, n_gates,
                                                      fill_value, out, s, ps, lanes_hint);
#define RG_K1P(IND_, NF_)                                                                                             \
  launch_nf<IND_, NF_, 384, true>(window_cap, indptr, nullptr, nullptr, dict_ptr, dict, cg, n_vox, packed, n_gates, \
                                  fill_value, out, s, ps)
  if (indptr_is_i64) {
    switch (n_fields) {
      case 1: return RG_K1P(int64_t, 1);
      case 2: return RG_K1P(int64_t, 2);
      case 3: return RG_K1P(int64_t, 3);
      default: return RG_K1P(int64_t, 4);
    }
  }
  switch (n_fields) {
    case 1: return RG_K1P(int32_t, 1);
    case 2: return RG_K1P(int32_t, 2);
    case 3: return RG_K1P(int32_t, 3);
    default: return RG_K1P(int32_t, 4);
  }
#undef RG_K1P
}

// ---------------------------------------------------------------------------------------------------------------
// Building the compact copy: the distinct gates of every chunk and each pair's position among them.
// One workgroup per chunk keeps an open-addressing hash set of gate indices in LDS.  Chunks whose dictionary would
// overload the table are processed in R = 2, 4, ... 32 rounds, round r taking the gates of one residue class of a
// second hash, so any chunk up to 65536 distinct gates is handled with 32 KiB of LDS.
//   count pass: distinct gates per chunk (and the rounds it needed)   -> rg_scan_counts_i64 gives dict_ptr
//   fill pass : same rounds; the lane that claims a slot gives the gate the next position and writes the dictionary
//               entry, a second sweep over the round's pairs looks every gate up and stores its 16-bit position.
// Positions depend on the insertion order (not reproducible run to run); the gridding result does not.
// `gate_idx` / `local_idx` are addressed by ABSOLUTE pair number (indptr values), so a caller that holds only a slab of
// the index array passes pointers shifted by the slab's first pair.
// ---------------------------------------------------------------------------------------------------------------
namespace {

constexpr int kSlots = 8192;          // hash slots per workgroup (32 KiB)
constexpr int kMaxLoad = 6144;        // distinct gates one round may insert
constexpr int kBuildThreads = 256;
constexpr int kMaxRounds = 32;
constexpr int kSplitFlag = 0x80;               // chunk_rounds bit: one dictionary per wavefront (see the apply kernel)
constexpr int kNotCompactable = 0x40000000;    // chunk_counts value: a single segment references > 65536 gates

__device__ __forceinline__ unsigned slot_hash(unsigned g) { return (g * 2654435761u) >> 19; }      // 13 bits
__device__ __forceinline__ unsigned round_hash(unsigned g) { return (g * 0x85EBCA6Bu) >> 27; }     // 5 bits

struct ChunkPairs {   // the (up to) H contiguous pair ranges of one chunk
  long p0[kH], p1[kH];
};

template <typename IndT>
__device__ __forceinline__ ChunkPairs chunk_pairs(const IndT* __restrict__ indptr, const ChunkGrid& cg, unsigned chunk) {
  ChunkPairs cp;
#pragma unroll
  for (int w = 0; w < kH; ++w) {
    const Segment s = chunk_segment(cg, chunk, w);
    cp.p0[w] = s.nrows ? (long)indptr[s.r0] : 0;
    cp.p1[w] = s.nrows ? (long)indptr[s.r0 + s.nrows] : 0;
  }
  return cp;
}

// Inserts the gates of residue class `r` (of `rounds`) among the chunk's pairs.  Returns false when the table overloads.
// With `ids`, the lane that claims a slot also gives the gate its position (base + order of arrival) and writes the
// dictionary entry: positions then follow the order in which the chunk's pairs first mention a gate, so the 64
// consecutive pairs of one gather mostly hold neighbouring positions (fewer LDS bank conflicts than any fixed order).
__device__ bool insert_round(const int32_t* __restrict__ gidx, const ChunkPairs& cp, int rounds, int r, int* table,
                             int* s_count, int* s_overflow, unsigned short* ids = nullptr, int base = 0,
                             int32_t* __restrict__ dict_out = nullptr, int room = 0) {
  for (int i = threadIdx.x; i < kSlots; i += kBuildThreads) table[i] = -1;
  if (threadIdx.x == 0) { *s_count = 0; *s_overflow = 0; }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kH; ++w) {
    for (long p = cp.p0[w] + threadIdx.x; p < cp.p1[w]; p += kBuildThreads) {
      const int g = gidx[p];
      if (rounds > 1 && (int)(round_hash((unsigned)g) & (unsigned)(rounds - 1)) != r) continue;
      unsigned h = slot_hash((unsigned)g);
      for (int probe = 0; probe < kSlots; ++probe) {   // bounded: a full table ends the walk (overflow is flagged first)
        const int seen = *(volatile int*)&table[h];   // other lanes insert concurrently
        if (seen == g) break;
        if (seen == -1) {
          if (*(volatile int*)s_overflow) break;
          const int old = atomicCAS(&table[h], -1, g);
          if (old == -1) {
            const int order = atomicAdd(s_count, 1);
            if (order >= kMaxLoad) *(volatile int*)s_overflow = 1;
            if (ids && base + order < room) {   // never writes past the dictionary the count pass sized
              ids[h] = (unsigned short)(base + order);
              dict_out[base + order] = g;
            }
            break;
          }
          if (old == g) break;
        }
        h = (h + 1) & (kSlots - 1);
      }
    }
  }
  __syncthreads();
  return *s_overflow == 0;
}

template <typename IndT>
__global__ __launch_bounds__(kBuildThreads) void compact_count_kernel(const IndT* __restrict__ indptr,
                                                                      const int32_t* __restrict__ gidx, ChunkGrid cg,
                                                                      int32_t* __restrict__ chunk_counts,
                                                                      uint8_t* __restrict__ chunk_rounds) {
  __shared__ int table[kSlots];
  __shared__ int s_count, s_overflow;
  const unsigned chunk = blockIdx.x;
  const ChunkPairs cp = chunk_pairs(indptr, cg, chunk);
  // distinct gates among the given ranges, and the hashing rounds that took (-1: more than kMaxRounds can hold)
  auto count = [&](const ChunkPairs& ranges, int& rounds) {
    int total = 0;
    while (true) {
      total = 0;
      bool ok = true;
      for (int r = 0; r < rounds && ok; ++r) {
        ok = insert_round(gidx, ranges, rounds, r, table, &s_count, &s_overflow);
        total += s_count;
        __syncthreads();
      }
      if (ok) return total;
      rounds *= 2;
      if (rounds > kMaxRounds) { rounds = kMaxRounds; return -1; }
    }
  };
  int rounds = 1;
  int total = count(cp, rounds);
  int flag = 0;
  if (total < 0 || total > 65536) {
    // too rich for 16-bit positions into ONE dictionary: one dictionary per wavefront (segment) instead, behind a
    // header of kH offsets.  rounds = the most any of the wavefronts needs.
    flag = kSplitFlag;
    total = kH;
    int worst = 1;
    for (int w = 0; w < kH; ++w) {
      ChunkPairs one;
#pragma unroll
      for (int k = 0; k < kH; ++k) { one.p0[k] = 0; one.p1[k] = 0; }
      one.p0[0] = cp.p0[w];
      one.p1[0] = cp.p1[w];
      int rw = 1;
      const int tw = count(one, rw);
      if (tw < 0 || tw > 65536) { total = kNotCompactable; break; }
      total += tw;
      worst = rw > worst ? rw : worst;
    }
    rounds = worst;
  }
  if (threadIdx.x == 0) {
    chunk_counts[chunk] = total;
    chunk_rounds[chunk] = (uint8_t)(rounds | flag);
  }
}

template <typename IndT>
__global__ __launch_bounds__(kBuildThreads) void compact_fill_kernel(const IndT* __restrict__ indptr,
                                                                     const int32_t* __restrict__ gidx, ChunkGrid cg,
                                                                     const int64_t* __restrict__ dict_ptr,
                                                                     const uint8_t* __restrict__ chunk_rounds,
                                                                     int32_t* __restrict__ dict,
                                                                     uint16_t* __restrict__ local_idx,
                                                                     int32_t* __restrict__ error_flag) {
  __shared__ int table[kSlots];
  __shared__ unsigned short ids[kSlots];
  __shared__ int s_count, s_overflow;
  const unsigned chunk = blockIdx.x;
  const ChunkPairs cp = chunk_pairs(indptr, cg, chunk);
  const long d0 = dict_ptr[chunk];
  const int expect = (int)(dict_ptr[chunk + 1] - d0);
  const int rounds = chunk_rounds[chunk] & (kSplitFlag - 1);
  const bool split = (chunk_rounds[chunk] & kSplitFlag) != 0;
  // positions of the given ranges' pairs into a dictionary written at dict_out; returns its size
  auto fill = [&](const ChunkPairs& ranges, int32_t* __restrict__ dict_out, int room) {
    int base = 0;
    for (int r = 0; r < rounds; ++r) {
      // cannot overload when the inputs are those of the count pass; if they are not (gate_idx changed in between, a
      // wrong chunk_rounds) the walks below are bounded and the mismatch is reported through error_flag, never a hang
      insert_round(gidx, ranges, rounds, r, table, &s_count, &s_overflow, ids, base, dict_out, room);
      if (threadIdx.x == 0 && (s_overflow || base + s_count > room)) atomicOr(error_flag, 1);
#pragma unroll
      for (int w = 0; w < kH; ++w) {
        for (long p = ranges.p0[w] + threadIdx.x; p < ranges.p1[w]; p += kBuildThreads) {
          const int g = gidx[p];
          if (rounds > 1 && (int)(round_hash((unsigned)g) & (unsigned)(rounds - 1)) != r) continue;
          unsigned h = slot_hash((unsigned)g);
          int probe = 0;
          while (table[h] != g && probe < kSlots) { h = (h + 1) & (kSlots - 1); ++probe; }
          if (probe == kSlots) {          // the gate was never inserted: count and fill saw different inputs
            atomicOr(error_flag, 2);
            local_idx[p] = 0;
          } else {
            local_idx[p] = ids[h];
          }
        }
      }
      base += s_count;
      __syncthreads();
    }
    return base;
  };
  int base;
  if (!split) {
    base = fill(cp, dict + d0, expect < 65536 ? expect : 65536);
  } else {
    base = kH;                                       // header: offset of every wavefront's dictionary
    for (int w = 0; w < kH; ++w) {
      if (threadIdx.x == 0) dict[d0 + w] = base;
      ChunkPairs one;
#pragma unroll
      for (int k = 0; k < kH; ++k) { one.p0[k] = 0; one.p1[k] = 0; }
      one.p0[0] = cp.p0[w];
      one.p1[0] = cp.p1[w];
      const int left = expect - base;
      base += fill(one, dict + d0 + base, left < 65536 ? (left > 0 ? left : 0) : 65536);
    }
  }
  if (threadIdx.x == 0 && base != expect) atomicOr(error_flag, 4);
}

}  // namespace

extern "C" int rg_csr_compact_count(const void* indptr, int32_t indptr_is_i64, const int32_t* gate_idx, int64_t n_rows,
                                    int64_t line_len, int64_t lines_per_plane, int32_t* chunk_counts,
                                    uint8_t* chunk_rounds, rg_stream_t stream) {
  RG_REQUIRE(n_rows >= 0, RG_EINVAL, "rg_csr_compact_count: negative size");
  if (n_rows == 0) return RG_OK;
  RG_REQUIRE(indptr && chunk_counts && chunk_rounds, RG_EINVAL, "rg_csr_compact_count: null pointer");
  ChunkGrid cg;
  RG_REQUIRE(make_chunk_grid(n_rows, line_len, lines_per_plane, &cg), RG_EINVAL,
             "rg_csr_compact_count: n_rows=%ld is not planes x lines_per_plane=%ld x line_len=%ld", (long)n_rows,
             (long)lines_per_plane, (long)line_len);
  const long chunks = chunk_count(cg);
  RG_REQUIRE(chunks <= 0x7FFFFFFFL, RG_EUNSUPPORTED, "rg_csr_compact_count: too many chunks for one launch");
  hipStream_t s = (hipStream_t)stream;
  if (indptr_is_i64)
    hipLaunchKernelGGL(compact_count_kernel<int64_t>, dim3((unsigned)chunks), dim3(kBuildThreads), 0, s,
                       static_cast<const int64_t*>(indptr), gate_idx, cg, chunk_counts, chunk_rounds);
  else
    hipLaunchKernelGGL(compact_count_kernel<int32_t>, dim3((unsigned)chunks), dim3(kBuildThreads), 0, s,
                       static_cast<const int32_t*>(indptr), gate_idx, cg, chunk_counts, chunk_rounds);
  return rg::check_launch("rg_csr_compact_count");
}

extern "C" int rg_csr_compact_fill(const void* indptr, int32_t indptr_is_i64, const int32_t* gate_idx, int64_t n_rows,
                                   int64_t line_len, int64_t lines_per_plane, const int64_t* dict_ptr,
                                   const uint8_t* chunk_rounds, int32_t* dict, uint16_t* local_idx, int32_t* error_flag,
                                   rg_stream_t stream) {
  RG_REQUIRE(n_rows >= 0, RG_EINVAL, "rg_csr_compact_fill: negative size");
  if (n_rows == 0) return RG_OK;
  RG_REQUIRE(indptr && dict_ptr && chunk_rounds && error_flag, RG_EINVAL, "rg_csr_compact_fill: null pointer");
  ChunkGrid cg;
  RG_REQUIRE(make_chunk_grid(n_rows, line_len, lines_per_plane, &cg), RG_EINVAL,
             "rg_csr_compact_fill: n_rows=%ld is not planes x lines_per_plane=%ld x line_len=%ld", (long)n_rows,
             (long)lines_per_plane, (long)line_len);
  const long chunks = chunk_count(cg);
  RG_REQUIRE(chunks <= 0x7FFFFFFFL, RG_EUNSUPPORTED, "rg_csr_compact_fill: too many chunks for one launch");
  hipStream_t s = (hipStream_t)stream;
  if (indptr_is_i64)
    hipLaunchKernelGGL(compact_fill_kernel<int64_t>, dim3((unsigned)chunks), dim3(kBuildThreads), 0, s,
                       static_cast<const int64_t*>(indptr), gate_idx, cg, dict_ptr, chunk_rounds, dict, local_idx,
                       error_flag);
  else
    hipLaunchKernelGGL(compact_fill_kernel<int32_t>, dim3((unsigned)chunks), dim3(kBuildThreads), 0, s,
                       static_cast<const int32_t*>(indptr), gate_idx, cg, dict_ptr, chunk_rounds, dict, local_idx,
                       error_flag);
  return rg::check_launch("rg_csr_compact_fill");
}
