// Building the compact CSR copy (layout: head of rg_csr_compact.hip): rg_csr_compact_count and rg_csr_compact_fill find the
// distinct gates of every chunk and each pair's position among them; rg_csr_row_ends16 writes the row-end table.
#include "rg_compact_layout.hpp"

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

// The row-end table the row-wise kernel reads instead of the row pointers (rg_csr_rowwise.hpp): one workgroup per grid line,
// one thread per row.  row_end16[v] = indptr[v + 1] - indptr[first row of v's segment]; every row of a segment whose span
// exceeds RG_ROW_END16_MAX gets RG_ROW_END16_WIDE (the kernel looks at the last one), so a table entry depends on the row
// pointers of its own segment alone -- a slab of whole planes writes what the whole grid would.
template <typename IndT>
__global__ __launch_bounds__(kBuildThreads) void row_ends16_kernel(const IndT* __restrict__ indptr, ChunkGrid cg,
                                                                   uint16_t* __restrict__ row_end16) {
  const long row0 = (long)blockIdx.x * cg.line_len;
  const unsigned split = cg.seg_extra * (cg.seg_base + 1);      // rows of a line that lie in the longer segments
  for (unsigned x = threadIdx.x; x < (unsigned)cg.line_len; x += kBuildThreads) {
    const unsigned sx = x < split ? x / (cg.seg_base + 1) : cg.seg_extra + (x - split) / cg.seg_base;
    const unsigned x0 = sx * cg.seg_base + (sx < cg.seg_extra ? sx : cg.seg_extra);
    const unsigned nrows = cg.seg_base + (sx < cg.seg_extra ? 1u : 0u);
    const long seg_b = (long)indptr[row0 + x0];
    const long span = (long)indptr[row0 + x0 + nrows] - seg_b;
    const long end = (long)indptr[row0 + x + 1] - seg_b;
    row_end16[row0 + x] = span <= RG_ROW_END16_MAX ? (uint16_t)end : (uint16_t)RG_ROW_END16_WIDE;
  }
}

}  // namespace

extern "C" int rg_csr_row_ends16(const void* indptr, int32_t indptr_is_i64, int64_t n_rows, int64_t line_len,
                                 int64_t lines_per_plane, uint16_t* row_end16, rg_stream_t stream) {
  RG_REQUIRE(n_rows >= 0, RG_EINVAL, "rg_csr_row_ends16: negative size");
  if (n_rows == 0) return RG_OK;
  RG_REQUIRE(indptr && row_end16, RG_EINVAL, "rg_csr_row_ends16: null pointer");
  ChunkGrid cg;
  RG_REQUIRE(make_chunk_grid(n_rows, line_len, lines_per_plane, &cg), RG_EINVAL,
             "rg_csr_row_ends16: n_rows=%ld is not planes x lines_per_plane=%ld x line_len=%ld", (long)n_rows,
             (long)lines_per_plane, (long)line_len);
  const long n_lines = cg.n_planes * cg.lines_per_plane;
  RG_REQUIRE(n_lines <= 0x7FFFFFFFL && cg.line_len <= 0x7FFFFFFFL, RG_EUNSUPPORTED, "rg_csr_row_ends16: too many lines for one launch");
  hipStream_t s = (hipStream_t)stream;
  if (indptr_is_i64)
    hipLaunchKernelGGL(row_ends16_kernel<int64_t>, dim3((unsigned)n_lines), dim3(kBuildThreads), 0, s,
                       static_cast<const int64_t*>(indptr), cg, row_end16);
  else
    hipLaunchKernelGGL(row_ends16_kernel<int32_t>, dim3((unsigned)n_lines), dim3(kBuildThreads), 0, s,
                       static_cast<const int32_t*>(indptr), cg, row_end16);
  return rg::check_launch("rg_csr_row_ends16");
}

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
