// K1c  csr_apply over a COMPACT device copy of the CSR.  Two families of kernels share the chunk layout, the
// dictionaries and the LDS field window described here:
//   * the TILE kernels (rg_csr_compact_apply_f32; rg_csr_compact_apply_packed_f32 with tile = 384), this file:
//     rg_csr_apply_f32's pipeline minus its gather stage -- the same results as rg_csr_apply_f32, bit for bit;
//   * the ROW-WISE kernel (rg_csr_compact_apply_packed_f32, tile = 0; rg_csr_rowwise.hpp): no LDS tile at all, the default
//     for passes of 1-4 fields -- the same results to float32 rounding, in an order of its own.
// rg_csr_compact_build.hip derives the copy from the standard CSR, rg_csr_pack.hip packs its positions and weights into records.
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

struct PackedStream {   // the packed form of positions + weights (rg_csr_compact_pack_dense); null = the plain arrays
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

}  // namespace

// The tile kernel over the packed records (declared in rg_compact_layout.hpp: rg_csr_rowwise.hip's entry point calls it).
int rg_launch_tile_packed(const StreamArgs& a, const ChunkGrid& cg) {
  const PackedStream ps{static_cast<const rg_u32x4*>(a.records), a.rec_ptr, a.w_base, a.rec_order};
  return rg::dispatch_index(a.is_i64, [&](auto ind) {
    return rg::dispatch_fields<4>(a.n_fields, [&](auto nf, auto) {
      return launch_nf<decltype(ind), decltype(nf)::value, 384, true>(a.window_cap, a.indptr, nullptr, nullptr, a.dict_ptr, a.dict,
                                                                      cg, a.n_vox, a.packed, a.n_gates, a.fill, a.out, a.stream, ps);
    });
  });
}

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
  // tiles (rg_row_phase.hpp's table): the defaults are the tiles rg_csr_apply_f32 uses for the same field count
  return rg::dispatch_index(indptr_is_i64 != 0, [&](auto ind) {
    return rg::dispatch_fields(n_fields, [&](auto nf, auto) {
      return rg::dispatch_tile<decltype(nf)::value>(tile, [&](auto tl) {
        return launch_nf<decltype(ind), decltype(nf)::value, decltype(tl)::value>(
            window_cap, indptr, local_idx, weights, dict_ptr, dict, cg, n_vox, packed, n_gates, fill_value, out, s);
      });
    });
  });
}
