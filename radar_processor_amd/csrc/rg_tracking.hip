// Cell overlap and tracking (include/radargrid_hip.h, "Cell overlap and tracking"): the contingency table of two label planes
// and the per-cell relabelling.
//
// Overlap is one pass with one thread per pixel.  A wavefront covers 64 consecutive flat indices, so the pixels of one pair
// (old cell, new cell) come in runs of lanes; a run's length is the distance between its first and its last lane, and only
// the last lane inserts.  The table is open addressing with linear probing in the caller's workspace:
//   keys    uint64 [C]   (row_prev << 32) | row_next, all ones = empty (rows stay below 2^31)
//   counts  int32  [C]   pixels of the pair
// A slot is claimed with one compare-and-swap; a thread that loses it looks at the key that won and either adds to it or moves
// on.  Nobody waits for anybody: the probe loop ends after C slots at the latest and then counts a dropped insertion.
//   clear    rg::fill_words over the table and totals (a kernel: see rg_common.hpp)
//   count    the pass over the pixels
//   compact  one thread per slot; occupied slots take an output index from totals[0], one atomic per wavefront
#include <limits.h>

#include "rg_common.hpp"
#include "rg_lane_runs.hpp"

namespace {

#define RG_TRK_RELAXED __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

constexpr unsigned long long kEmpty = ~0ull;
constexpr int64_t kMaxPairs = (int64_t)1 << 30;             // exclusive: C = 2 * max_pairs rounded up stays below 2^31

// smallest power of two >= max(2 * max_pairs, 64)
inline int64_t capacity_of(int64_t max_pairs) {
  int64_t c = 64;
  while (c < 2 * max_pairs) c <<= 1;
  return c;
}

// the finaliser of splitmix64: every bit of the key reaches the low bits that pick the slot
__device__ __forceinline__ unsigned long long mix(unsigned long long k) {
  k ^= k >> 30;
  k *= 0xBF58476D1CE4E5B9ull;
  k ^= k >> 27;
  k *= 0x94D049BB133111EBull;
  k ^= k >> 31;
  return k;
}

// the row of a CellTable pixel i of plane p belongs to, or -1: background, a label above the plane's cell count, or a row
// that would not fit 31 bits (a cell_ptr that no labelling writes)
__device__ __forceinline__ int row_of(const int* __restrict__ labels, const int* __restrict__ cell_ptr, long i, long p) {
  const int l = labels[i];
  if (l <= 0) return -1;
  const long first = cell_ptr[p], cells = (long)cell_ptr[p + 1] - first;
  const long row = first + l - 1;
  return l <= cells && row >= 0 && row <= INT_MAX ? (int)row : -1;
}

__global__ __launch_bounds__(rg::kBlock) void overlap_count_kernel(const int* __restrict__ labels_prev,
                                                                   const int* __restrict__ ptr_prev,
                                                                   const int* __restrict__ labels_next,
                                                                   const int* __restrict__ ptr_next, long hw, long n,
                                                                   unsigned capacity_mask, unsigned long long* keys, int* counts,
                                                                   int* totals) {
  const long i = (long)blockIdx.x * rg::kBlock + threadIdx.x;
  const int lane = threadIdx.x % rg::kWave;
  int a = -1, b = -1;
  if (i < n) {
    const long p = i / hw;
    a = row_of(labels_prev, ptr_prev, i, p);
    b = a >= 0 ? row_of(labels_next, ptr_next, i, p) : -1;
    if (b < 0) a = -1;                                        // one of the two is background: no pair
  }
  if (__ballot(a >= 0) == 0ull) return;
  int start;
  bool tail;
  rg::run_of_pair(a, b, lane, &start, &tail);
  if (!tail || a < 0) return;
  const int count = lane - start + 1;                         // every lane of a run holds one pixel
  const unsigned long long key = ((unsigned long long)(unsigned)a << 32) | (unsigned)b;
  unsigned slot = (unsigned)mix(key) & capacity_mask;
  for (unsigned probe = 0; probe <= capacity_mask; ++probe) {
    unsigned long long seen = __hip_atomic_load(keys + slot, RG_TRK_RELAXED);
    if (seen == kEmpty) {
      // on failure `seen` becomes the key that claimed the slot first
      if (__hip_atomic_compare_exchange_strong(keys + slot, &seen, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT))
        seen = key;
    }
    if (seen == key) {
      __hip_atomic_fetch_add(counts + slot, count, RG_TRK_RELAXED);
      return;
    }
    slot = (slot + 1u) & capacity_mask;
  }
  __hip_atomic_fetch_add(totals + 1, 1, RG_TRK_RELAXED);      // every slot holds another pair: dropped
}

__global__ __launch_bounds__(rg::kBlock) void overlap_compact_kernel(const unsigned long long* __restrict__ keys,
                                                                     const int* __restrict__ counts, long capacity,
                                                                     long max_pairs, int* __restrict__ pair_rows,
                                                                     int* __restrict__ pair_count, int* totals) {
  const long s = (long)blockIdx.x * rg::kBlock + threadIdx.x;
  const int lane = threadIdx.x % rg::kWave;
  const unsigned long long key = s < capacity ? keys[s] : kEmpty;
  const unsigned long long held = __ballot(key != kEmpty);
  if (held == 0ull) return;
  const int leader = __builtin_ctzll(held);
  int base = 0;
  if (lane == leader) base = __hip_atomic_fetch_add(totals, __builtin_popcountll(held), RG_TRK_RELAXED);
  base = __shfl(base, leader);
  if (key == kEmpty) return;
  const long at = (long)base + __builtin_popcountll(held & ((1ull << lane) - 1ull));
  if (at >= max_pairs) return;
  pair_rows[2 * at] = (int)(key >> 32);
  pair_rows[2 * at + 1] = (int)(key & 0xFFFFFFFFull);
  pair_count[at] = counts[s];
}

__global__ __launch_bounds__(rg::kBlock) void relabel_kernel(const int* labels, const int* __restrict__ cell_ptr,
                                                             const int* __restrict__ lut, long hw, long n, int n_cells,
                                                             int* out) {
  const long i = (long)blockIdx.x * rg::kBlock + threadIdx.x;
  if (i >= n) return;
  const int row = n_cells > 0 ? row_of(labels, cell_ptr, i, i / hw) : -1;
  out[i] = row >= 0 && row < n_cells ? lut[row] : 0;
}

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

inline unsigned blocks_for(long n) { return (unsigned)((n + rg::kBlock - 1) / rg::kBlock); }

// sizes both entry points share: 0 <= n_planes * h * w < 2^31
int check_sizes(const char* who, int32_t n_planes, int32_t h, int32_t w) {
  RG_REQUIRE(n_planes >= 1, RG_EINVAL, "%s: n_planes must be at least 1, got %d", who, n_planes);
  RG_REQUIRE(h >= 0 && w >= 0, RG_EINVAL, "%s: negative size %d x %d", who, h, w);
  RG_REQUIRE((__int128)n_planes * h * w < ((__int128)1 << 31), RG_EINVAL, "%s: %d planes of %d x %d are 2^31 pixels or more", who,
             n_planes, h, w);
  return RG_OK;
}

}  // namespace

extern "C" int64_t rg_cell_overlap_workspace_bytes(int64_t max_pairs) {
  RG_REQUIRE(max_pairs >= 1 && max_pairs < kMaxPairs, RG_EINVAL,
             "rg_cell_overlap_workspace_bytes: max_pairs must lie in 1 .. 2^30 - 1, got %lld", (long long)max_pairs);
  return capacity_of(max_pairs) * 12;                        // keys, then counts; C >= 64 keeps it a multiple of 16
}

extern "C" int rg_cell_overlap_i32(const int32_t* labels_prev, const int32_t* cell_ptr_prev, const int32_t* labels_next,
                                   const int32_t* cell_ptr_next, int32_t n_planes, int32_t h, int32_t w, int64_t max_pairs,
                                   int32_t* pair_rows, int32_t* pair_count, int32_t* totals, void* workspace,
                                   int64_t workspace_bytes, rg_stream_t stream) {
  const char* who = "rg_cell_overlap_i32";
  const int status = check_sizes(who, n_planes, h, w);
  if (status != RG_OK) return status;
  RG_REQUIRE(max_pairs >= 1 && max_pairs < kMaxPairs, RG_EINVAL, "%s: max_pairs must lie in 1 .. 2^30 - 1, got %lld", who,
             (long long)max_pairs);
  RG_REQUIRE(labels_prev && cell_ptr_prev && labels_next && cell_ptr_next && pair_rows && pair_count && totals && workspace,
             RG_EINVAL, "%s: null pointer", who);
  RG_REQUIRE(aligned_to(labels_prev, 4) && aligned_to(cell_ptr_prev, 4) && aligned_to(labels_next, 4) &&
                 aligned_to(cell_ptr_next, 4) && aligned_to(pair_rows, 4) && aligned_to(pair_count, 4) && aligned_to(totals, 4) &&
                 aligned_to(workspace, 8),
             RG_EALIGN, "%s: the int32 arrays must be 4-byte aligned, the workspace 8-byte aligned", who);
  const int64_t need = rg_cell_overlap_workspace_bytes(max_pairs);
  RG_REQUIRE(workspace_bytes >= need, RG_EWORKSPACE, "%s: workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes,
             (long long)need);
  const long hw = (long)h * w, n = n_planes * hw;
  const int64_t label_bytes = n * 4, ptr_bytes = ((int64_t)n_planes + 1) * 4;
  const struct { const void* p; int64_t bytes; } ins[] = {{labels_prev, label_bytes}, {labels_next, label_bytes},
                                                           {cell_ptr_prev, ptr_bytes}, {cell_ptr_next, ptr_bytes}},
      outs[] = {{pair_rows, max_pairs * 8}, {pair_count, max_pairs * 4}, {totals, 8}, {workspace, need}};
  for (const auto& o : outs)
    for (const auto& in : ins)
      RG_REQUIRE(!rg::overlap(o.p, o.bytes, in.p, in.bytes), RG_EINVAL, "%s: an output or the workspace overlaps an input", who);
  hipStream_t s = (hipStream_t)stream;
  rg::fill_words(totals, 8, 0u, s);
  if (n == 0) return rg::check_launch(who);
  const int64_t capacity = capacity_of(max_pairs);
  unsigned long long* keys = static_cast<unsigned long long*>(workspace);
  int* counts = reinterpret_cast<int*>(keys + capacity);
  rg::fill_words(keys, capacity * 8, 0xFFFFFFFFu, s);
  rg::fill_words(counts, capacity * 4, 0u, s);
  hipLaunchKernelGGL(overlap_count_kernel, dim3(blocks_for(n)), dim3(rg::kBlock), 0, s, labels_prev, cell_ptr_prev, labels_next,
                     cell_ptr_next, hw, n, (unsigned)(capacity - 1), keys, counts, totals);
  hipLaunchKernelGGL(overlap_compact_kernel, dim3(blocks_for(capacity)), dim3(rg::kBlock), 0, s, keys, counts, (long)capacity,
                     (long)max_pairs, pair_rows, pair_count, totals);
  return rg::check_launch(who);
}

extern "C" int rg_relabel_cells_i32(const int32_t* labels, const int32_t* cell_ptr, int32_t n_planes, int32_t h, int32_t w,
                                    const int32_t* lut, int32_t n_cells, int32_t* out, rg_stream_t stream) {
  const char* who = "rg_relabel_cells_i32";
  const int status = check_sizes(who, n_planes, h, w);
  if (status != RG_OK) return status;
  RG_REQUIRE(n_cells >= 0, RG_EINVAL, "%s: negative n_cells %d", who, n_cells);
  const long hw = (long)h * w, n = n_planes * hw;
  if (n == 0) return RG_OK;
  RG_REQUIRE(labels && cell_ptr && out && (lut || n_cells == 0), RG_EINVAL, "%s: null pointer", who);
  RG_REQUIRE(aligned_to(labels, 4) && aligned_to(cell_ptr, 4) && aligned_to(lut, 4) && aligned_to(out, 4), RG_EALIGN,
             "%s: an array is not 4-byte aligned", who);
  RG_REQUIRE(out == labels || !rg::overlap(out, n * 4, labels, n * 4), RG_EINVAL, "%s: out overlaps labels without being labels",
             who);
  RG_REQUIRE(!rg::overlap(out, n * 4, cell_ptr, ((int64_t)n_planes + 1) * 4) &&
                 (n_cells == 0 || !rg::overlap(out, n * 4, lut, (int64_t)n_cells * 4)),
             RG_EINVAL, "%s: out overlaps cell_ptr or lut", who);
  hipLaunchKernelGGL(relabel_kernel, dim3(blocks_for(n)), dim3(rg::kBlock), 0, (hipStream_t)stream, labels, cell_ptr, lut, hw, n,
                     n_cells, out);
  return rg::check_launch(who);
}
