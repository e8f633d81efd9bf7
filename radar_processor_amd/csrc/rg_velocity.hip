// Doppler velocity dealiasing by regions (include/radargrid_velocity.h): the band split, the flattening of the labelling, the
// region adjacency table and the per-region fold.
//
// Three of the four kernels are pointwise.  The adjacency table is the one with a hot path: one thread per pixel, a wavefront
// covers 64 consecutive flat indices, and the pixel pairs across a border between two regions come in runs of lanes with one
// key (lo << 32 | hi).  A run is summed with a segmented shuffle scan -- the count is the run's length, the difference an int64
// -- and only its last lane inserts into the table, which is rg_tracking.hip's: open addressing with linear probing in the
// caller's workspace,
//   keys    uint64 [C]   lo << 32 | hi, all ones = empty (ids stay below 2^31)
//   sums    int64  [C]   sum of q(hi pixel) - q(lo pixel)
//   counts  int32  [C]   pixel pairs of the edge
// A slot is claimed with one compare-and-swap; a thread that loses it looks at the key that won and either adds to it or moves
// on.  Nobody waits for anybody: the probe loop ends after C slots at the latest and then counts a dropped insertion.
//   clear    rg::fill_words over the table and totals (a kernel: see rg_common.hpp)
//   count    the pass over the pixels, right neighbours first, then the neighbours below (the wrap seam among them)
//   compact  one thread per slot; occupied slots take an output index from totals[0], one atomic per wavefront
#include <math.h>

#include "radargrid_velocity.h"
#include "rg_common.hpp"
#include "rg_lane_runs.hpp"

namespace {

#define RG_VEL_RELAXED __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

constexpr unsigned long long kEmpty = ~0ull;
constexpr int64_t kMaxEdges = (int64_t)1 << 30;             // exclusive: C = 2 * max_edges rounded up stays below 2^31
constexpr uint32_t kQuietNaN = 0x7FC00000u;

// the Nyquist velocities of the sweeps of one launch, passed by value: nothing of the host array outlives the call
struct Nyquists {
  double v[RG_VELOCITY_SWEEPS_PER_LAUNCH];
};

// smallest power of two >= max(2 * max_edges, 64)
inline int64_t capacity_of(int64_t max_edges) {
  int64_t c = 64;
  while (c < 2 * max_edges) c <<= 1;
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

// finite and |v| <= RG_VELOCITY_MAX_ABS: both fail for NaN, the second for +-inf
__device__ __forceinline__ bool valid_value(float v) { return fabsf(v) <= (float)RG_VELOCITY_MAX_ABS; }

// q = llrint(65536 * v): the product is exact in float64, the rounding is to nearest even
__device__ __forceinline__ long long fixed_point(float v) { return llrint(65536.0 * (double)v); }

// ---- 1  split ------------------------------------------------------------------------------------------------------------------
// gates: R * G; n: the gates of this launch's sweeps; vel, mask and split begin at the launch's first sweep
__global__ __launch_bounds__(rg::kBlock) void split_kernel(const float* __restrict__ vel, const uint8_t* __restrict__ mask,
                                                           Nyquists nyq, long gates, long n, int n_bands,
                                                           float* __restrict__ split) {
  const long i = (long)blockIdx.x * rg::kBlock + threadIdx.x;
  if (i >= n) return;
  const long s = i / gates, g = i - s * gates;
  const float v = vel[i];
  int band = -1;
  if (valid_value(v) && !(mask && mask[i])) {
    const double vn = nyq.v[s];
    const double t = floor(((double)v + vn) * n_bands / (2.0 * vn));
    band = t < 0.0 ? 0 : t > (double)(n_bands - 1) ? n_bands - 1 : (int)t;
  }
  float* plane = split + s * n_bands * gates + g;
  for (int b = 0; b < n_bands; ++b) plane[b * gates] = b == band ? v : rg::bits_f32(kQuietNaN);
}

// ---- 2  regions ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(rg::kBlock) void regions_kernel(const int* __restrict__ labels, const int* __restrict__ cell_ptr,
                                                             long gates, long n, int n_bands, int* __restrict__ regions) {
  const long i = (long)blockIdx.x * rg::kBlock + threadIdx.x;
  if (i >= n) return;
  const long s = i / gates, g = i - s * gates;
  int id = 0;
  for (int b = 0; b < n_bands && id == 0; ++b) {
    const long plane = s * n_bands + b;
    const int l = labels[plane * gates + g];
    if (l <= 0) continue;
    const int first = cell_ptr[plane];
    if ((long)l <= (long)cell_ptr[plane + 1] - first) id = first + l;
  }
  regions[i] = id;
}

// ---- 3  region edges -----------------------------------------------------------------------------------------------------------
// Every lane of the wavefront calls this.  Lanes without an edge hold the key (-1, -1) and a zero difference; they form runs of
// their own and insert nothing.
__device__ __forceinline__ void insert_runs(bool edge, int lo, int hi, long long diff, int lane, unsigned capacity_mask,
                                            unsigned long long* keys, long long* sums, int* counts, int* totals) {
  int start;
  bool tail;
  rg::run_of_pair(lo, hi, lane, &start, &tail);
#pragma unroll
  for (int d = 1; d < rg::kWave; d <<= 1) {                   // segmented inclusive scan: a lane only takes from its own run
    const long long t = __shfl_up(diff, d);
    if (lane - d >= start) diff += t;
  }
  if (tail && edge) {
    const int count = lane - start + 1;                       // every lane of a run holds one pixel pair
    const unsigned long long key = ((unsigned long long)(unsigned)lo << 32) | (unsigned)hi;
    unsigned slot = (unsigned)mix(key) & capacity_mask;
    bool placed = false;
    for (unsigned probe = 0; probe <= capacity_mask && !placed; ++probe) {
      unsigned long long seen = __hip_atomic_load(keys + slot, RG_VEL_RELAXED);
      if (seen == kEmpty) {
        // on failure `seen` becomes the key that claimed the slot first
        if (__hip_atomic_compare_exchange_strong(keys + slot, &seen, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
          seen = key;
      }
      if (seen == key) {
        __hip_atomic_fetch_add(counts + slot, count, RG_VEL_RELAXED);
        __hip_atomic_fetch_add(sums + slot, diff, RG_VEL_RELAXED);
        placed = true;
      }
      slot = (slot + 1u) & capacity_mask;
    }
    if (!placed) __hip_atomic_fetch_add(totals + 1, 1, RG_VEL_RELAXED);   // every slot holds another edge: dropped
  }
}

__global__ __launch_bounds__(rg::kBlock) void region_edges_kernel(const float* __restrict__ values,
                                                                  const int* __restrict__ regions, int h, int w, long hw, long n,
                                                                  int wrap_rows, unsigned capacity_mask,
                                                                  unsigned long long* keys, long long* sums, int* counts,
                                                                  int* totals) {
  const long i = (long)blockIdx.x * rg::kBlock + threadIdx.x;
  const int lane = threadIdx.x % rg::kWave;
  int a = 0, y = 0, x = 0;
  if (i < n) {
    a = regions[i];
    const long at = i % hw;
    y = (int)(at / w);
    x = (int)(at - (long)y * w);
  }
  if (__ballot(a > 0) == 0ull) return;                        // no region in these 64 pixels: no edge begins here
  for (int dir = 0; dir < 2; ++dir) {
    long j = -1;                                              // the forward neighbour of this direction, or none
    if (a > 0) {
      if (dir == 0) {
        if (x + 1 < w) j = i + 1;
      } else if (y + 1 < h) {
        j = i + w;
      } else if (wrap_rows && h >= 3) {
        j = i - (long)(h - 1) * w;                            // y == h - 1: row 0 of the same plane
      }
    }
    bool edge = false;
    int lo = -1, hi = -1;
    long long diff = 0;
    if (j >= 0) {
      const int b = regions[j];
      if (b > 0 && b != a) {                                  // values are read only where two regions meet
        const float va = values[i], vb = values[j];
        if (valid_value(va) && valid_value(vb)) {
          edge = true;
          lo = a < b ? a : b;
          hi = a < b ? b : a;
          diff = a < b ? fixed_point(vb) - fixed_point(va) : fixed_point(va) - fixed_point(vb);
        }
      }
    }
    if (__ballot(edge) == 0ull) continue;
    insert_runs(edge, lo, hi, diff, lane, capacity_mask, keys, sums, counts, totals);
  }
}

__global__ __launch_bounds__(rg::kBlock) void edges_compact_kernel(const unsigned long long* __restrict__ keys,
                                                                   const long long* __restrict__ sums,
                                                                   const int* __restrict__ counts, long capacity, long max_edges,
                                                                   int* __restrict__ pair_ids, int* __restrict__ pair_count,
                                                                   long long* __restrict__ pair_sum, int* totals) {
  const long s = (long)blockIdx.x * rg::kBlock + threadIdx.x;
  const int lane = threadIdx.x % rg::kWave;
  const unsigned long long key = s < capacity ? keys[s] : kEmpty;
  const unsigned long long held = __ballot(key != kEmpty);
  if (held == 0ull) return;
  const int leader = __builtin_ctzll(held);
  int base = 0;
  if (lane == leader) base = __hip_atomic_fetch_add(totals, __builtin_popcountll(held), RG_VEL_RELAXED);
  base = __shfl(base, leader);
  if (key == kEmpty) return;
  const long at = (long)base + __builtin_popcountll(held & ((1ull << lane) - 1ull));
  if (at >= max_edges) return;
  pair_ids[2 * at] = (int)(key >> 32);
  pair_ids[2 * at + 1] = (int)(key & 0xFFFFFFFFull);
  pair_count[at] = counts[s];
  pair_sum[at] = sums[s];
}

// ---- 4  apply ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(rg::kBlock) void apply_folds_kernel(const float* vel, const int* __restrict__ regions,
                                                                 const int* __restrict__ fold_lut, int n_regions, Nyquists nyq,
                                                                 long gates, long n, float* out, int* __restrict__ folds) {
  const long i = (long)blockIdx.x * rg::kBlock + threadIdx.x;
  if (i >= n) return;
  const int id = regions[i];
  float result = rg::bits_f32(kQuietNaN);
  int f = 0;
  if (id > 0 && id <= n_regions) {
    f = fold_lut[id - 1];
    result = (float)((double)vel[i] + (double)f * (2.0 * nyq.v[i / gates]));
    if (result != result) {
      result = rg::bits_f32(kQuietNaN);
      f = 0;
    }
  }
  out[i] = result;
  if (folds) folds[i] = f;
}

// ---- host --------------------------------------------------------------------------------------------------------------------
struct Span {
  const void* p;
  int64_t bytes;
  const char* name;
};

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

inline unsigned blocks_for(long n) { return (unsigned)((n + rg::kBlock - 1) / rg::kBlock); }

// S, R >= 1, G >= 0 and S * planes_per_sweep * R * G < 2^31
int check_volume(const char* who, int32_t S, int32_t R, int32_t G, int32_t planes_per_sweep) {
  RG_REQUIRE(S >= 1 && R >= 1, RG_EINVAL, "%s: S and R must be at least 1, got %d and %d", who, S, R);
  RG_REQUIRE(G >= 0, RG_EINVAL, "%s: G must not be negative, got %d", who, G);
  RG_REQUIRE((__int128)S * planes_per_sweep * R * G < ((__int128)1 << 31), RG_EINVAL,
             "%s: %d sweeps x %d plane(s) of %d x %d are 2^31 gates or more", who, S, planes_per_sweep, R, G);
  return RG_OK;
}

int check_bands(const char* who, int32_t n_bands) {
  RG_REQUIRE(n_bands >= RG_VELOCITY_MIN_BANDS && n_bands <= RG_VELOCITY_MAX_BANDS, RG_EINVAL, "%s: n_bands must lie in %d .. %d, got %d",
             who, RG_VELOCITY_MIN_BANDS, RG_VELOCITY_MAX_BANDS, n_bands);
  return RG_OK;
}

int check_nyquist(const char* who, const double* nyquist_host, int32_t S) {
  for (int32_t s = 0; s < S; ++s)
    RG_REQUIRE(isfinite(nyquist_host[s]) && nyquist_host[s] > 0.0 && nyquist_host[s] <= (double)RG_VELOCITY_MAX_NYQUIST, RG_EINVAL,
               "%s: the Nyquist velocity of sweep %d must be finite with 0 < Vn <= %d, got %g", who, s, RG_VELOCITY_MAX_NYQUIST,
               nyquist_host[s]);
  return RG_OK;
}

// no output overlaps an input or another output, except that output a may EQUAL the input of index same[a] (-1: none)
int check_overlaps(const char* who, const Span* in, int n_in, const Span* out, const int* same, int n_out) {
  for (int a = 0; a < n_out; ++a) {
    if (!out[a].p) continue;
    for (int b = 0; b < n_in; ++b) {
      if (!in[b].p || (same[a] == b && out[a].p == in[b].p)) continue;
      RG_REQUIRE(!rg::overlap(out[a].p, out[a].bytes, in[b].p, in[b].bytes), RG_EINVAL, "%s: %s overlaps %s", who, out[a].name,
                 in[b].name);
    }
    for (int b = a + 1; b < n_out; ++b)
      RG_REQUIRE(!(out[b].p && rg::overlap(out[a].p, out[a].bytes, out[b].p, out[b].bytes)), RG_EINVAL, "%s: %s overlaps %s", who,
                 out[a].name, out[b].name);
  }
  return RG_OK;
}

// the Nyquist velocities of the sweeps first .. first + count - 1; the rest of the array repeats the last (never read)
Nyquists nyquists_of(const double* nyquist_host, int32_t first, int32_t count) {
  Nyquists nyq;
  for (int k = 0; k < RG_VELOCITY_SWEEPS_PER_LAUNCH; ++k) nyq.v[k] = nyquist_host[first + (k < count ? k : count - 1)];
  return nyq;
}

}  // namespace

extern "C" int rg_velocity_split_f32(const float* vel, const uint8_t* mask, int32_t S, int32_t R, int32_t G,
                                     const double* nyquist_host, int32_t n_bands, float* split, rg_stream_t stream) {
  const char* who = "rg_velocity_split_f32";
  RG_REQUIRE(vel && nyquist_host && split, RG_EINVAL, "%s: null pointer", who);
  int status = check_bands(who, n_bands);
  if (status == RG_OK) status = check_volume(who, S, R, G, n_bands);
  if (status == RG_OK) status = check_nyquist(who, nyquist_host, S);
  if (status != RG_OK) return status;
  const long gates = (long)R * G;
  const int64_t n = (int64_t)S * gates;
  const Span in[] = {{vel, n * 4, "vel"}, {mask, n, "mask"}};
  const Span outs[] = {{split, n * n_bands * 4, "split"}};
  const int same[] = {-1};
  status = check_overlaps(who, in, 2, outs, same, 1);
  if (status != RG_OK) return status;
  if (G == 0) return RG_OK;
  for (int32_t first = 0; first < S; first += RG_VELOCITY_SWEEPS_PER_LAUNCH) {
    const int32_t count = S - first < RG_VELOCITY_SWEEPS_PER_LAUNCH ? S - first : RG_VELOCITY_SWEEPS_PER_LAUNCH;
    const long at = first * gates, here = count * gates;
    hipLaunchKernelGGL(split_kernel, dim3(blocks_for(here)), dim3(rg::kBlock), 0, (hipStream_t)stream, vel + at,
                       mask ? mask + at : nullptr, nyquists_of(nyquist_host, first, count), gates, here, n_bands,
                       split + at * n_bands);
  }
  return rg::check_launch(who);
}

extern "C" int rg_velocity_regions_i32(const int32_t* labels, const int32_t* cell_ptr, int32_t S, int32_t R, int32_t G,
                                       int32_t n_bands, int32_t* regions, rg_stream_t stream) {
  const char* who = "rg_velocity_regions_i32";
  RG_REQUIRE(labels && cell_ptr && regions, RG_EINVAL, "%s: null pointer", who);
  int status = check_bands(who, n_bands);
  if (status == RG_OK) status = check_volume(who, S, R, G, n_bands);
  if (status != RG_OK) return status;
  const long gates = (long)R * G;
  const int64_t n = (int64_t)S * gates;
  const Span in[] = {{labels, n * n_bands * 4, "labels"}, {cell_ptr, ((int64_t)S * n_bands + 1) * 4, "cell_ptr"}};
  const Span outs[] = {{regions, n * 4, "regions"}};
  const int same[] = {-1};
  status = check_overlaps(who, in, 2, outs, same, 1);
  if (status != RG_OK) return status;
  if (G == 0) return RG_OK;
  hipLaunchKernelGGL(regions_kernel, dim3(blocks_for(n)), dim3(rg::kBlock), 0, (hipStream_t)stream, labels, cell_ptr, gates, (long)n,
                     n_bands, regions);
  return rg::check_launch(who);
}

extern "C" int64_t rg_region_edges_workspace_bytes(int64_t max_edges) {
  RG_REQUIRE(max_edges >= 1 && max_edges < kMaxEdges, RG_EINVAL,
             "rg_region_edges_workspace_bytes: max_edges must lie in 1 .. 2^30 - 1, got %lld", (long long)max_edges);
  return capacity_of(max_edges) * 20;                        // keys, sums, counts; C >= 64 keeps it a multiple of 16
}

extern "C" int rg_region_edges_f32(const float* values, const int32_t* regions, int32_t n_planes, int32_t h, int32_t w,
                                   int32_t wrap_rows, int64_t max_edges, int32_t* pair_ids, int32_t* pair_count, int64_t* pair_sum,
                                   int32_t* totals, void* workspace, int64_t workspace_bytes, rg_stream_t stream) {
  const char* who = "rg_region_edges_f32";
  RG_REQUIRE(n_planes >= 1, RG_EINVAL, "%s: n_planes must be at least 1, got %d", who, n_planes);
  RG_REQUIRE(h >= 0 && w >= 0, RG_EINVAL, "%s: negative size %d x %d", who, h, w);
  RG_REQUIRE((__int128)n_planes * h * w < ((__int128)1 << 31), RG_EINVAL, "%s: %d planes of %d x %d are 2^31 pixels or more", who,
             n_planes, h, w);
  RG_REQUIRE(max_edges >= 1 && max_edges < kMaxEdges, RG_EINVAL, "%s: max_edges must lie in 1 .. 2^30 - 1, got %lld", who,
             (long long)max_edges);
  RG_REQUIRE(values && regions && pair_ids && pair_count && pair_sum && totals && workspace, RG_EINVAL, "%s: null pointer", who);
  RG_REQUIRE(aligned_to(values, 4) && aligned_to(regions, 4) && aligned_to(pair_ids, 4) && aligned_to(pair_count, 4) &&
                 aligned_to(totals, 4) && aligned_to(pair_sum, 8) && aligned_to(workspace, 8),
             RG_EALIGN, "%s: the 32-bit arrays must be 4-byte aligned, pair_sum and the workspace 8-byte aligned", who);
  const int64_t need = rg_region_edges_workspace_bytes(max_edges);
  RG_REQUIRE(workspace_bytes >= need, RG_EWORKSPACE, "%s: workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes,
             (long long)need);
  const long hw = (long)h * w, n = n_planes * hw;
  const Span in[] = {{values, n * 4, "values"}, {regions, n * 4, "regions"}};
  const Span outs[] = {{pair_ids, max_edges * 8, "pair_ids"}, {pair_count, max_edges * 4, "pair_count"},
                       {pair_sum, max_edges * 8, "pair_sum"}, {totals, 8, "totals"}, {workspace, need, "workspace"}};
  for (const Span& o : outs)
    for (const Span& i : in)
      RG_REQUIRE(!rg::overlap(o.p, o.bytes, i.p, i.bytes), RG_EINVAL, "%s: %s overlaps %s", who, o.name, i.name);
  hipStream_t s = (hipStream_t)stream;
  rg::fill_words(totals, 8, 0u, s);
  if (n == 0) return rg::check_launch(who);
  const int64_t capacity = capacity_of(max_edges);
  unsigned long long* keys = static_cast<unsigned long long*>(workspace);
  long long* sums = reinterpret_cast<long long*>(keys + capacity);
  int* counts = reinterpret_cast<int*>(sums + capacity);
  rg::fill_words(keys, capacity * 8, 0xFFFFFFFFu, s);
  rg::fill_words(sums, capacity * 12, 0u, s);                 // the sums and, behind them, the counts
  hipLaunchKernelGGL(region_edges_kernel, dim3(blocks_for(n)), dim3(rg::kBlock), 0, s, values, regions, h, w, hw, n, wrap_rows,
                     (unsigned)(capacity - 1), keys, sums, counts, totals);
  hipLaunchKernelGGL(edges_compact_kernel, dim3(blocks_for(capacity)), dim3(rg::kBlock), 0, s, keys, sums, counts, (long)capacity,
                     (long)max_edges, pair_ids, pair_count, reinterpret_cast<long long*>(pair_sum), totals);
  return rg::check_launch(who);
}

extern "C" int rg_velocity_apply_folds_f32(const float* vel, const int32_t* regions, const int32_t* fold_lut, int32_t n_regions,
                                           int32_t S, int32_t R, int32_t G, const double* nyquist_host, float* out, int32_t* folds,
                                           rg_stream_t stream) {
  const char* who = "rg_velocity_apply_folds_f32";
  RG_REQUIRE(vel && regions && nyquist_host && out, RG_EINVAL, "%s: null pointer", who);
  RG_REQUIRE(n_regions >= 0, RG_EINVAL, "%s: negative n_regions %d", who, n_regions);
  RG_REQUIRE(fold_lut || n_regions == 0, RG_EINVAL, "%s: null pointer", who);
  int status = check_volume(who, S, R, G, 1);
  if (status == RG_OK) status = check_nyquist(who, nyquist_host, S);
  if (status != RG_OK) return status;
  const long gates = (long)R * G;
  const int64_t n = (int64_t)S * gates;
  const Span in[] = {{vel, n * 4, "vel"}, {regions, n * 4, "regions"}, {fold_lut, (int64_t)n_regions * 4, "fold_lut"}};
  const Span outs[] = {{out, n * 4, "out"}, {folds, n * 4, "folds"}};
  const int same[] = {0, -1};
  status = check_overlaps(who, in, 3, outs, same, 2);
  if (status != RG_OK) return status;
  if (G == 0) return RG_OK;
  for (int32_t first = 0; first < S; first += RG_VELOCITY_SWEEPS_PER_LAUNCH) {
    const int32_t count = S - first < RG_VELOCITY_SWEEPS_PER_LAUNCH ? S - first : RG_VELOCITY_SWEEPS_PER_LAUNCH;
    const long at = first * gates, here = count * gates;
    hipLaunchKernelGGL(apply_folds_kernel, dim3(blocks_for(here)), dim3(rg::kBlock), 0, (hipStream_t)stream, vel + at, regions + at,
                       fold_lut, n_regions, nyquists_of(nyquist_host, first, count), gates, here, out + at,
                       folds ? folds + at : nullptr);
  }
  return rg::check_launch(who);
}
