// Connected echo regions (include/radargrid_hip.h, "Connected echo regions"): labelling, the per-cell table, despeckling.
//
// Labelling is a union-find over pixels in which the LARGER root is always linked under the SMALLER one, so parent[i] <= i
// holds at every moment, `find` walks strictly decreasing indices (it terminates whatever other threads do meanwhile) and
// the root a cell ends with is its smallest flat index: its first pixel in raster order.  Ranking the roots in index order
// is then scipy.ndimage.label's numbering, without a sort.
//   tile     one workgroup per RG_CC_TILE_H x RG_CC_TILE_W tile, union-find in LDS.  A wavefront takes a tile row as ONE
//            ballot: a pixel starts under the first pixel of its run, so only vertical links need a union.
//   seam     one thread per pixel next to a tile border (and per pixel of row 0 under wrap_rows) unites it with its
//            neighbours across the border: agent-scope atomic minima, retried on the value they return; every read that
//            steers a union is a relaxed agent-scope atomic load (a plain one may see another XCD's stale line).
//   flatten  every pixel -> its root, into `labels` (parent is only read); roots counted per chunk of kChunk pixels
//   scan     one workgroup turns the chunk counts into running offsets and writes cell_ptr
//   rank     roots get their id (rank within the plane + 1), written over parent[root]
//   write    labels[i] = parent[labels[i]]
// The phases are separate launches on the caller's stream; no workgroup ever waits for another.
#include <limits.h>
#include <math.h>
#include <string.h>

#include "rg_common.hpp"
#include "rg_lane_runs.hpp"

namespace {

constexpr int kTH = RG_CC_TILE_H, kTW = RG_CC_TILE_W;
constexpr int kWaves = rg::kBlock / rg::kWave;
constexpr int kPerThread = 4;                                   // consecutive pixels of one thread in flatten / rank
constexpr int kChunk = rg::kBlock * kPerThread;                 // pixels of one workgroup there: the unit of the scan
static_assert(kTW == rg::kWave, "a tile row is one wavefront's ballot");
static_assert(kTH % kWaves == 0, "every wavefront takes the same number of tile rows");

#define RG_CC_RELAXED __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// ---- tile pass ---------------------------------------------------------------------------------------------------------------
// lab[] only ever decreases (atomicMin), so a stale read is a valid ancestor: volatile keeps the loop re-reading
__device__ __forceinline__ int find_lds(volatile int* lab, int a) {
  for (int p = lab[a]; p != a; p = lab[a]) a = p;
  return a;
}

__device__ __forceinline__ void unite_lds(int* lab, int a, int b) {
  for (;;) {
    a = find_lds(lab, a);
    b = find_lds(lab, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(&lab[a], b);      // a > b: link the larger root under the smaller
    if (old == a) return;                       // a was still a root: linked
    a = old;                                    // somebody linked a first (old < a): unite what it hangs under with b
  }
}

__global__ __launch_bounds__(rg::kBlock) void cc_tile_kernel(const float* __restrict__ src, const uint8_t* __restrict__ mask,
                                                             int h, int w, float lo, float hi, int conn8, int tiles_x,
                                                             int tiles_y, int* __restrict__ parent) {
  __shared__ int lab[kTH * kTW];
  __shared__ unsigned long long rows[kTH];
  const int tiles = tiles_x * tiles_y;
  const int p = blockIdx.x / tiles, t = blockIdx.x - p * tiles;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int lane = threadIdx.x % rg::kWave, wave = threadIdx.x / rg::kWave;
  const int x = tx * kTW + lane;
  const size_t plane = (size_t)p * h * w;
  for (int r = wave; r < kTH; r += kWaves) {
    const int y = ty * kTH + r;
    bool fg = false;
    if (y < h && x < w) {
      const size_t i = plane + (size_t)y * w + x;
      const float v = src[i];
      fg = v >= lo && v <= hi && (mask == nullptr || mask[i] == 0);
    }
    const unsigned long long m = __ballot(fg);
    if (lane == 0) rows[r] = m;
    const unsigned long long gaps = ~m & ((1ull << lane) - 1ull);          // background pixels to my left
    const int start = gaps ? 64 - __builtin_clzll(gaps) : 0;              // first pixel of my run
    lab[r * kTW + lane] = fg ? r * kTW + start : -1;
  }
  __syncthreads();
  for (int r = wave; r < kTH; r += kWaves) {
    if (r == 0) continue;
    const unsigned long long m = rows[r], up = rows[r - 1];
    if (!((m >> lane) & 1ull)) continue;
    const bool west = lane > 0 && ((m >> (lane - 1)) & 1ull);
    const bool n = (up >> lane) & 1ull;
    const bool nw = lane > 0 && ((up >> (lane - 1)) & 1ull);
    const bool ne = lane < kTW - 1 && ((up >> (lane + 1)) & 1ull);
    const int i = r * kTW + lane;
    // a link is skipped where the pixel to the west (same run) already made it: west and north-west both foreground
    if (n) {
      if (!(west && nw)) unite_lds(lab, i, i - kTW);
    } else if (conn8) {
      if (nw && !west) unite_lds(lab, i, i - kTW - 1);
      if (ne) unite_lds(lab, i, i - kTW + 1);
    }
  }
  __syncthreads();
  for (int r = wave; r < kTH; r += kWaves) {
    const int y = ty * kTH + r;
    if (y >= h || x >= w) continue;
    const size_t i = plane + (size_t)y * w + x;
    int root = -1;
    if (lab[r * kTW + lane] >= 0) {
      const int l = find_lds(lab, r * kTW + lane);
      root = (int)(plane + (size_t)(ty * kTH + l / kTW) * w + (tx * kTW + l % kTW));
    }
    parent[i] = root;
  }
}

// ---- seam pass ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int load_agent(int* p) { return __hip_atomic_load(p, RG_CC_RELAXED); }

__device__ __forceinline__ int find_global(int* parent, int a) {
  int r = a;
  for (int p = load_agent(parent + r); p != r; p = load_agent(parent + r)) r = p;
  if (r != a) __hip_atomic_fetch_min(parent + a, r, RG_CC_RELAXED);      // shorten the path: r is an ancestor, r < parent[a]
  return r;
}

__device__ __forceinline__ void unite_global(int* parent, int a, int b) {
  for (;;) {
    a = find_global(parent, a);
    b = find_global(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = __hip_atomic_fetch_min(parent + a, b, RG_CC_RELAXED);
    if (old == a) return;
    a = old;
  }
}

// pixel `a` (foreground) against the pixel at (y, x) of its plane, if that is inside and foreground
__device__ __forceinline__ void seam_pair(int* parent, int a, long plane, int y, int x, int h, int w) {
  if (y < 0 || y >= h || x < 0 || x >= w) return;
  const int b = (int)(plane + (long)y * w + x);
  if (load_agent(parent + b) >= 0) unite_global(parent, a, b);
}

// per plane: n_hs rows of w threads (the rows below a horizontal tile border; last, row 0 against row h - 1 under wrap), then
// n_vs columns of h threads (the columns right of a vertical border)
__global__ __launch_bounds__(rg::kBlock) void cc_seam_kernel(int* parent, int h, int w, int conn8, int tiles_y, int n_hs,
                                                             int n_vs, long per_plane, long total) {
  const long t = (long)blockIdx.x * rg::kBlock + threadIdx.x;
  if (t >= total) return;
  const long p = t / per_plane;
  long u = t - p * per_plane;
  const long plane = p * (long)h * w;
  if (u < (long)n_hs * w) {
    const int s = (int)(u / w), x = (int)(u - (long)s * w);
    const int y = s < tiles_y - 1 ? (s + 1) * kTH : 0;
    const int yn = s < tiles_y - 1 ? y - 1 : h - 1;
    const int a = (int)(plane + (long)y * w + x);
    if (load_agent(parent + a) < 0) return;
    seam_pair(parent, a, plane, yn, x, h, w);
    if (conn8) {
      seam_pair(parent, a, plane, yn, x - 1, h, w);
      seam_pair(parent, a, plane, yn, x + 1, h, w);
    }
  } else {
    u -= (long)n_hs * w;
    const int s = (int)(u / h), y = (int)(u - (long)s * h);
    const int x = (s + 1) * kTW;
    const int a = (int)(plane + (long)y * w + x);
    if (load_agent(parent + a) < 0) return;
    seam_pair(parent, a, plane, y, x - 1, h, w);
    if (conn8) {
      seam_pair(parent, a, plane, y - 1, x - 1, h, w);
      seam_pair(parent, a, plane, y + 1, x - 1, h, w);
    }
  }
}

// ---- flatten, scan, rank, write ----------------------------------------------------------------------------------------------
// exclusive prefix of v over the workgroup's threads; *total = the sum.  Two barriers: callable in a loop.
__device__ __forceinline__ int block_exclusive_scan(int v, int* total) {
  __shared__ int wave_sum[kWaves];
  const int lane = threadIdx.x % rg::kWave, wave = threadIdx.x / rg::kWave;
  int incl = v;
#pragma unroll
  for (int d = 1; d < rg::kWave; d <<= 1) {
    const int o = __shfl_up(incl, d);
    if (lane >= d) incl += o;
  }
  __syncthreads();
  if (lane == rg::kWave - 1) wave_sum[wave] = incl;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < kWaves; ++k) {
    const int s = wave_sum[k];
    if (k < wave) before += s;
    all += s;
  }
  *total = all;
  return before + incl - v;
}

// chunk c of plane p = blockIdx.x: pixels [c * kChunk, min((c + 1) * kChunk, hw)) of the plane, kPerThread consecutive ones
// per thread
__global__ __launch_bounds__(rg::kBlock) void cc_flatten_kernel(const int* __restrict__ parent, long hw, int chunks,
                                                                int* __restrict__ root, int* __restrict__ counts) {
  const long p = blockIdx.x / chunks, c = blockIdx.x - p * chunks;
  const long first = c * kChunk + (long)threadIdx.x * kPerThread;
  int mine = 0;
  for (int k = 0; k < kPerThread; ++k) {
    const long j = first + k;
    if (j >= hw) break;
    const long i = p * hw + j;
    int r = parent[i];
    if (r >= 0) {
      for (int q = parent[r]; q != r; q = parent[r]) r = q;
      mine += r == (int)i;
    }
    root[i] = r;
  }
  int total;
  block_exclusive_scan(mine, &total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// one workgroup: counts[n] -> exclusive running sums in place; cell_ptr[p] = the sum before plane p's first chunk
__global__ __launch_bounds__(rg::kBlock) void cc_scan_kernel(int* __restrict__ counts, long n, int chunks, long n_planes,
                                                             int* __restrict__ cell_ptr) {
  int carry = 0;
  for (long base = 0; base < n; base += rg::kBlock) {
    const long b = base + threadIdx.x;
    const int v = b < n ? counts[b] : 0;
    int total;
    const int excl = carry + block_exclusive_scan(v, &total);
    if (b < n) {
      counts[b] = excl;
      if (b % chunks == 0) cell_ptr[b / chunks] = excl;
    }
    carry += total;
  }
  if (threadIdx.x == 0) cell_ptr[n_planes] = carry;
}

__global__ __launch_bounds__(rg::kBlock) void cc_rank_kernel(const int* __restrict__ root, const int* __restrict__ offsets,
                                                             long hw, int chunks, int* __restrict__ ids) {
  const long p = blockIdx.x / chunks, c = blockIdx.x - p * chunks;
  const long first = c * kChunk + (long)threadIdx.x * kPerThread;
  bool is_root[kPerThread];
  int mine = 0;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const long j = first + k;
    is_root[k] = j < hw && root[p * hw + j] == (int)(p * hw + j);
    mine += is_root[k];
  }
  int total;
  int rank = block_exclusive_scan(mine, &total) + offsets[blockIdx.x] - offsets[p * chunks];
#pragma unroll
  for (int k = 0; k < kPerThread; ++k)
    if (is_root[k]) ids[p * hw + first + k] = ++rank;
}

__global__ __launch_bounds__(rg::kBlock) void cc_write_kernel(const int* __restrict__ ids, long n, int* __restrict__ labels) {
  const long i = (long)blockIdx.x * rg::kBlock + threadIdx.x;
  if (i >= n) return;
  const int r = labels[i];
  labels[i] = r >= 0 ? ids[r] : 0;
}

// ---- the cell table ----------------------------------------------------------------------------------------------------------
// order-preserving map of a non-NaN float's bits: larger value <=> larger key; never 0 (0 would be the bits of a NaN)
__device__ __forceinline__ uint32_t order_key(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ __forceinline__ uint32_t key_bits(uint32_t key) { return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu); }
constexpr uint32_t kNoKey = 0u;
constexpr uint32_t kNanBits = 0x7FC00000u;

// runs of equal `cell` among the wavefront's lanes: start = first lane of my run, tail = I am its last lane
using rg::run_of;

__device__ __forceinline__ long shfl_up_i64(long v, int d) {
  const int lo = __shfl_up((int)(v & 0xFFFFFFFFl), d), hi = __shfl_up((int)(v >> 32), d);
  return ((long)hi << 32) | (unsigned int)lo;
}

__global__ __launch_bounds__(rg::kBlock) void cc_stats_init_kernel(int n_cells, int* area, int* bbox, long* sum_yx,
                                                                   uint32_t* vmax_key, int* argmax, double* vsum) {
  const int c = blockIdx.x * rg::kBlock + threadIdx.x;
  if (c >= n_cells) return;
  if (area) area[c] = 0;
  if (bbox) {
    bbox[4 * c + 0] = INT_MAX;
    bbox[4 * c + 1] = -1;
    bbox[4 * c + 2] = INT_MAX;
    bbox[4 * c + 3] = -1;
  }
  if (sum_yx) sum_yx[2 * c] = sum_yx[2 * c + 1] = 0;
  if (vmax_key) vmax_key[c] = kNoKey;
  if (argmax) argmax[c] = INT_MAX;
  if (vsum) vsum[c] = 0.0;
}

// the row of the per-cell arrays pixel i belongs to, or -1 (background, or a label beyond n_cells)
__device__ __forceinline__ int cell_of(const int* __restrict__ labels, const int* __restrict__ cell_ptr, long i, long p,
                                       int n_cells) {
  const int l = labels[i];
  if (l <= 0) return -1;
  const long c = (long)cell_ptr[p] + l - 1;
  return c < n_cells ? (int)c : -1;
}

// one thread per pixel; a wavefront is 64 consecutive flat indices, so the pixels of a cell come in runs of lanes.  Each run
// is combined with a segmented scan (a lane only ever takes from lanes of its own run) and its last lane issues the atomics.
__global__ __launch_bounds__(rg::kBlock) void cc_stats_kernel(const float* __restrict__ src, const int* __restrict__ labels,
                                                              const int* __restrict__ cell_ptr, long hw, int w, long n,
                                                              int n_cells, int* area, int* bbox, long* sum_yx,
                                                              uint32_t* vmax_key, double* vsum) {
  const long i = (long)blockIdx.x * rg::kBlock + threadIdx.x;
  const int lane = threadIdx.x % rg::kWave;
  int cell = -1, y = 0, x = 0;
  float v = 0.0f;
  if (i < n) {
    const long p = i / hw, j = i - p * hw;
    cell = cell_of(labels, cell_ptr, i, p, n_cells);
    y = (int)(j / w);
    x = (int)(j - (long)y * w);
    if (cell >= 0) v = src[i];
  }
  if (__ballot(cell >= 0) == 0ull) return;
  int start;
  bool tail;
  run_of(cell, lane, &start, &tail);
  int count = 1, y0 = y, y1 = y, x0 = x, x1 = x;
  long sy = y, sx = x;
  uint32_t key = isnan(v) ? kNoKey : order_key(rg::f32_bits(v));
  double vs = (double)v;
#pragma unroll
  for (int d = 1; d < rg::kWave; d <<= 1) {
    const int o_count = __shfl_up(count, d), o_y0 = __shfl_up(y0, d), o_y1 = __shfl_up(y1, d), o_x0 = __shfl_up(x0, d),
              o_x1 = __shfl_up(x1, d);
    const long o_sy = shfl_up_i64(sy, d), o_sx = shfl_up_i64(sx, d);
    const uint32_t o_key = (uint32_t)__shfl_up((int)key, d);
    const double o_vs = __shfl_up(vs, d);
    if (lane - d >= start) {
      count += o_count;
      y0 = min(y0, o_y0);
      y1 = max(y1, o_y1);
      x0 = min(x0, o_x0);
      x1 = max(x1, o_x1);
      sy += o_sy;
      sx += o_sx;
      key = max(key, o_key);
      vs = o_vs + vs;
    }
  }
  if (!tail || cell < 0) return;
  if (area) atomicAdd(area + cell, count);
  if (bbox) {
    atomicMin(bbox + 4 * cell + 0, y0);
    atomicMax(bbox + 4 * cell + 1, y1);
    atomicMin(bbox + 4 * cell + 2, x0);
    atomicMax(bbox + 4 * cell + 3, x1);
  }
  if (sum_yx) {
    atomicAdd(reinterpret_cast<unsigned long long*>(sum_yx + 2 * cell), (unsigned long long)sy);
    atomicAdd(reinterpret_cast<unsigned long long*>(sum_yx + 2 * cell + 1), (unsigned long long)sx);
  }
  if (vmax_key && key != kNoKey) atomicMax(vmax_key + cell, key);
  if (vsum) atomicAdd(vsum + cell, vs);
}

// second step of argmax: the pixels that hold their cell's maximum take the smallest index (one atomic minimum per run)
__global__ __launch_bounds__(rg::kBlock) void cc_argmax_kernel(const float* __restrict__ src, const int* __restrict__ labels,
                                                               const int* __restrict__ cell_ptr, long hw, long n, int n_cells,
                                                               const uint32_t* __restrict__ vmax_key, int* argmax) {
  const long i = (long)blockIdx.x * rg::kBlock + threadIdx.x;
  const int lane = threadIdx.x % rg::kWave;
  int cell = -1, at = INT_MAX;
  if (i < n) {
    const long p = i / hw;
    cell = cell_of(labels, cell_ptr, i, p, n_cells);
    if (cell >= 0) {
      const float v = src[i];
      if (!isnan(v) && order_key(rg::f32_bits(v)) == vmax_key[cell]) at = (int)(i - p * hw);
    }
  }
  if (__ballot(at != INT_MAX) == 0ull) return;
  int start;
  bool tail;
  run_of(cell, lane, &start, &tail);
#pragma unroll
  for (int d = 1; d < rg::kWave; d <<= 1) {
    const int o = __shfl_up(at, d);
    if (lane - d >= start) at = min(at, o);
  }
  if (tail && cell >= 0 && at != INT_MAX) atomicMin(argmax + cell, at);
}

__global__ __launch_bounds__(rg::kBlock) void cc_stats_finish_kernel(int n_cells, uint32_t* vmax_key, int* argmax) {
  const int c = blockIdx.x * rg::kBlock + threadIdx.x;
  if (c >= n_cells) return;
  const uint32_t key = vmax_key[c];
  vmax_key[c] = key == kNoKey ? kNanBits : key_bits(key);
  if (argmax && argmax[c] == INT_MAX) argmax[c] = -1;
}

// ---- despeckle ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(rg::kBlock) void cc_select_kernel(const uint32_t* src, const int* __restrict__ labels,
                                                               const int* __restrict__ cell_ptr, const int* __restrict__ area,
                                                               long hw, long n, int min_size, uint32_t fill, uint32_t* out,
                                                               uint8_t* __restrict__ out_mask) {
  const long i = (long)blockIdx.x * rg::kBlock + threadIdx.x;
  if (i >= n) return;
  const int l = labels[i];
  const bool removed = l > 0 && area[cell_ptr[i / hw] + l - 1] < min_size;
  out[i] = removed ? fill : src[i];
  if (out_mask) out_mask[i] = removed ? 1 : 0;
}

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

inline unsigned blocks_for(long n) { return (unsigned)((n + rg::kBlock - 1) / rg::kBlock); }

// sizes every entry point shares: 0 <= n_planes * h * w < 2^31
int check_sizes(const char* who, int32_t n_planes, int32_t h, int32_t w) {
  RG_REQUIRE(n_planes >= 1, RG_EINVAL, "%s: n_planes must be at least 1, got %d", who, n_planes);
  RG_REQUIRE(h >= 0 && w >= 0, RG_EINVAL, "%s: negative size %d x %d", who, h, w);
  RG_REQUIRE((__int128)n_planes * h * w < ((__int128)1 << 31), RG_EINVAL, "%s: %d planes of %d x %d are 2^31 pixels or more", who,
             n_planes, h, w);
  return RG_OK;
}

inline long chunks_of(long hw) { return (hw + kChunk - 1) / kChunk; }

}  // namespace

extern "C" int64_t rg_components_workspace_bytes(int32_t n_planes, int32_t h, int32_t w) {
  const int status = check_sizes("rg_components_workspace_bytes", n_planes, h, w);
  if (status != RG_OK) return status;
  const long hw = (long)h * w;
  const long words = n_planes * hw + n_planes * chunks_of(hw);        // parent / ids, then the chunk counts
  return (words * 4 + 15) / 16 * 16;
}

extern "C" int rg_label_components_f32(const float* src, const uint8_t* mask, int32_t n_planes, int32_t h, int32_t w, float lo,
                                       float hi, int32_t connectivity, int32_t wrap_rows, int32_t* labels, int32_t* cell_ptr,
                                       void* workspace, int64_t workspace_bytes, rg_stream_t stream) {
  const char* who = "rg_label_components_f32";
  const int status = check_sizes(who, n_planes, h, w);
  if (status != RG_OK) return status;
  RG_REQUIRE(cell_ptr, RG_EINVAL, "%s: null cell_ptr", who);
  RG_REQUIRE(!isnan(lo) && !isnan(hi), RG_EINVAL, "%s: lo and hi must not be NaN", who);
  RG_REQUIRE(connectivity == 4 || connectivity == 8, RG_EINVAL, "%s: connectivity must be 4 or 8, got %d", who, connectivity);
  RG_REQUIRE(aligned_to(cell_ptr, 4), RG_EALIGN, "%s: cell_ptr must be 4-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  const long hw = (long)h * w, n = n_planes * hw;
  if (n == 0) {
    rg::fill_words(cell_ptr, ((int64_t)n_planes + 1) * 4, 0u, s);
    return rg::check_launch(who);
  }
  RG_REQUIRE(src && labels && workspace, RG_EINVAL, "%s: null pointer", who);
  RG_REQUIRE(aligned_to(src, 4) && aligned_to(labels, 4) && aligned_to(workspace, 4), RG_EALIGN,
             "%s: src, labels and workspace must be 4-byte aligned", who);
  RG_REQUIRE(workspace_bytes >= rg_components_workspace_bytes(n_planes, h, w), RG_EWORKSPACE,
             "%s: workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes,
             (long long)rg_components_workspace_bytes(n_planes, h, w));
  const uintptr_t a = reinterpret_cast<uintptr_t>(src), b = reinterpret_cast<uintptr_t>(labels);
  RG_REQUIRE(a + (uintptr_t)n * 4 <= b || b + (uintptr_t)n * 4 <= a, RG_EINVAL, "%s: labels overlaps src", who);
  const int conn8 = connectivity == 8;
  const int tiles_x = (w + kTW - 1) / kTW, tiles_y = (h + kTH - 1) / kTH;
  const long chunks = chunks_of(hw), n_chunks = n_planes * chunks;            // both < 2^31: n is
  int* parent = static_cast<int*>(workspace);
  int* counts = parent + n;
  // tiles <= n / 1 and n < 2^31, so the tile count fits a grid dimension
  hipLaunchKernelGGL(cc_tile_kernel, dim3((unsigned)((long)n_planes * tiles_x * tiles_y)), dim3(rg::kBlock), 0, s, src, mask, h, w,
                     lo, hi, conn8, tiles_x, tiles_y, parent);
  const int n_hs = tiles_y - 1 + (wrap_rows ? 1 : 0), n_vs = tiles_x - 1;
  const long per_plane = (long)n_hs * w + (long)n_vs * h;
  if (per_plane > 0)
    hipLaunchKernelGGL(cc_seam_kernel, dim3(blocks_for(n_planes * per_plane)), dim3(rg::kBlock), 0, s, parent, h, w, conn8, tiles_y,
                       n_hs, n_vs, per_plane, n_planes * per_plane);
  hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned)n_chunks), dim3(rg::kBlock), 0, s, parent, hw, (int)chunks, labels, counts);
  hipLaunchKernelGGL(cc_scan_kernel, dim3(1), dim3(rg::kBlock), 0, s, counts, n_chunks, (int)chunks, (long)n_planes, cell_ptr);
  hipLaunchKernelGGL(cc_rank_kernel, dim3((unsigned)n_chunks), dim3(rg::kBlock), 0, s, labels, counts, hw, (int)chunks, parent);
  hipLaunchKernelGGL(cc_write_kernel, dim3(blocks_for(n)), dim3(rg::kBlock), 0, s, parent, n, labels);
  return rg::check_launch(who);
}

extern "C" int rg_component_stats_f32(const float* src, const int32_t* labels, const int32_t* cell_ptr, int32_t n_planes,
                                      int32_t h, int32_t w, int32_t n_cells, int32_t* area, int32_t* bbox, int64_t* sum_yx,
                                      float* vmax, int32_t* argmax, double* vsum, rg_stream_t stream) {
  const char* who = "rg_component_stats_f32";
  const int status = check_sizes(who, n_planes, h, w);
  if (status != RG_OK) return status;
  RG_REQUIRE(n_cells >= 0, RG_EINVAL, "%s: negative n_cells %d", who, n_cells);
  RG_REQUIRE(!argmax || vmax, RG_EINVAL, "%s: argmax needs vmax", who);
  const long hw = (long)h * w, n = n_planes * hw;
  if (n_cells == 0 || n == 0) return RG_OK;
  RG_REQUIRE(src && labels && cell_ptr, RG_EINVAL, "%s: null pointer", who);
  RG_REQUIRE(aligned_to(src, 4) && aligned_to(labels, 4) && aligned_to(cell_ptr, 4) && aligned_to(area, 4) &&
                 aligned_to(bbox, 4) && aligned_to(sum_yx, 8) && aligned_to(vmax, 4) && aligned_to(argmax, 4) &&
                 aligned_to(vsum, 8),
             RG_EALIGN, "%s: an array is not aligned to its element size", who);
  hipStream_t s = (hipStream_t)stream;
  uint32_t* key = reinterpret_cast<uint32_t*>(vmax);
  long* sums = reinterpret_cast<long*>(sum_yx);
  hipLaunchKernelGGL(cc_stats_init_kernel, dim3(blocks_for(n_cells)), dim3(rg::kBlock), 0, s, n_cells, area, bbox, sums, key, argmax,
                     vsum);
  hipLaunchKernelGGL(cc_stats_kernel, dim3(blocks_for(n)), dim3(rg::kBlock), 0, s, src, labels, cell_ptr, hw, w, n, n_cells, area,
                     bbox, sums, key, vsum);
  if (argmax)
    hipLaunchKernelGGL(cc_argmax_kernel, dim3(blocks_for(n)), dim3(rg::kBlock), 0, s, src, labels, cell_ptr, hw, n, n_cells, key,
                       argmax);
  if (vmax)
    hipLaunchKernelGGL(cc_stats_finish_kernel, dim3(blocks_for(n_cells)), dim3(rg::kBlock), 0, s, n_cells, key, argmax);
  return rg::check_launch(who);
}

extern "C" int rg_despeckle_select_f32(const float* src, const int32_t* labels, const int32_t* cell_ptr, const int32_t* area,
                                       int32_t n_planes, int32_t h, int32_t w, int32_t min_size, float fill, float* out,
                                       uint8_t* out_mask, rg_stream_t stream) {
  const char* who = "rg_despeckle_select_f32";
  const int status = check_sizes(who, n_planes, h, w);
  if (status != RG_OK) return status;
  RG_REQUIRE(min_size >= 1, RG_EINVAL, "%s: min_size must be at least 1, got %d", who, min_size);
  const long hw = (long)h * w, n = n_planes * hw;
  if (n == 0) return RG_OK;
  RG_REQUIRE(src && labels && cell_ptr && area && out, RG_EINVAL, "%s: null pointer", who);
  RG_REQUIRE(aligned_to(src, 4) && aligned_to(labels, 4) && aligned_to(cell_ptr, 4) && aligned_to(area, 4) && aligned_to(out, 4),
             RG_EALIGN, "%s: an array is not 4-byte aligned", who);
  uint32_t fill_bits;
  memcpy(&fill_bits, &fill, sizeof fill_bits);
  hipLaunchKernelGGL(cc_select_kernel, dim3(blocks_for(n)), dim3(rg::kBlock), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint32_t*>(src), labels, cell_ptr, area, hw, n, min_size, fill_bits,
                     reinterpret_cast<uint32_t*>(out), out_mask);
  return rg::check_launch(who);
}
