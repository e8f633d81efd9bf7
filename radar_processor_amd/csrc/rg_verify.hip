// Nowcast verification (include/radargrid_hip.h, "Nowcast verification"): contingency counts at thresholds, the summed-area
// tables of the threshold exceedances, the three sums of the fractions skill score over a ladder of window sizes, and the
// neighbourhood exceedance fraction.
//
// Everything here is an integer: a pixel exceeds a threshold or it does not, a window count is four table entries, and the
// sums are 64-bit integer adds -- so the order in which wavefronts and workgroups arrive shows in nothing, and every output is
// bit-reproducible although three of the four kernels end in atomics.
//   contingency   grid-stride over the pixels of one plane; one read of forecast, observation and mask serves all thresholds;
//                 per threshold three ballots, whose popcounts are wave-uniform and accumulate in scalar registers; the four
//                 wavefronts meet in LDS and the workgroup issues one atomic per counter
//   SAT, rows     one wavefront per row, 64 pixels per trip: the predicate is one bit, so the ballot IS the scan --
//                 popcount(ballot & lanes up to me) + carry -- without a shuffle ladder or LDS
//   SAT, columns  one thread per (layer, column) adds down the rows in place, kColumnUnroll loads in flight ahead of the adds
//   FSS sums      one workgroup per (strip of pixels, layer, scale): eight table reads per pixel, three 64-bit accumulators per
//                 thread, shuffles, LDS, three atomics per workgroup; at most kMaxStrips workgroups add into one word
//   fraction      one thread per pixel, four table reads, one float64 division
#include <math.h>

#include <algorithm>

#include "rg_common.hpp"

namespace {

#define RG_VER_RELAXED __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

constexpr int kWavesPerBlock = rg::kBlock / rg::kWave;
constexpr int kMaxStrips = 1024;          // workgroups per (layer, scale) or per plane: the atomics one word receives
constexpr int kColumnUnroll = 8;          // rows whose loads the column pass issues before it adds them
constexpr int kLayersPerLaunch = 32768;   // gridDim.y of the FSS launch; more layers take further launches
constexpr int kCounters = 3 * RG_MAX_VERIFY_THRESHOLDS + 1;

// thresholds by value: wave-uniform, read from scalar registers.  Entries from n on are NaN, which nothing exceeds.
struct Thresholds {
  float t[RG_MAX_VERIFY_THRESHOLDS];
};

struct Scales {
  int n[RG_MAX_VERIFY_SCALES];
};

__device__ __forceinline__ unsigned long long lanes_up_to(int lane) { return ~0ull >> (63 - lane); }

// ---- contingency -------------------------------------------------------------------------------------------------------------
// blockIdx.y = the plane, blockIdx.x = the strip; every wavefront walks whole groups of 64 pixels, so the ballots see all lanes
__global__ __launch_bounds__(rg::kBlock) void contingency_kernel(const float* __restrict__ fcst, const float* __restrict__ obs,
                                                                 const uint8_t* __restrict__ mask, int hw, Thresholds thr,
                                                                 int n_thr, long long* counts, long long* valid_out) {
  __shared__ unsigned part[kWavesPerBlock][kCounters];
  const int lane = threadIdx.x % rg::kWave, wave = threadIdx.x / rg::kWave;
  const size_t plane = (size_t)blockIdx.y * (size_t)hw;
  unsigned acc[kCounters];
#pragma unroll
  for (int c = 0; c < kCounters; ++c) acc[c] = 0u;
  const long step = (long)gridDim.x * rg::kBlock;
  for (long base = (long)blockIdx.x * rg::kBlock + wave * rg::kWave; base < hw; base += step) {
    const long i = base + lane;
    float f = 0.0f, o = 0.0f;
    bool ok = i < hw;
    if (ok) {
      f = fcst[plane + i];
      o = obs[plane + i];
      ok = !isnan(f) && !isnan(o) && !(mask && mask[plane + i]);
    }
    acc[kCounters - 1] += (unsigned)__builtin_popcountll(__ballot(ok));
#pragma unroll
    for (int t = 0; t < RG_MAX_VERIFY_THRESHOLDS; ++t) {
      if (t < n_thr) {
        const bool fe = ok && f >= thr.t[t], oe = ok && o >= thr.t[t];
        acc[3 * t] += (unsigned)__builtin_popcountll(__ballot(fe && oe));
        acc[3 * t + 1] += (unsigned)__builtin_popcountll(__ballot(fe && !oe));
        acc[3 * t + 2] += (unsigned)__builtin_popcountll(__ballot(!fe && oe));
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < kCounters; ++c) part[wave][c] = acc[c];
  }
  __syncthreads();
  const int c = threadIdx.x;
  if (c < 3 * n_thr || c == kCounters - 1) {
    unsigned long long total = 0;
#pragma unroll
    for (int v = 0; v < kWavesPerBlock; ++v) total += part[v][c];
    if (total) {
      long long* to = c == kCounters - 1 ? valid_out + blockIdx.y : counts + (size_t)blockIdx.y * 3 * n_thr + c;
      __hip_atomic_fetch_add(to, (long long)total, RG_VER_RELAXED);
    }
  }
}

// ---- summed-area table: rows -------------------------------------------------------------------------------------------------
// one wavefront per row of one plane; writes the inclusive row prefix of every threshold's exceedance bit
__global__ __launch_bounds__(rg::kBlock) void sat_rows_kernel(const float* __restrict__ src, const float* __restrict__ partner,
                                                              const uint8_t* __restrict__ mask, long rows, int h, int w,
                                                              Thresholds thr, int n_thr, int* __restrict__ sat) {
  const int lane = threadIdx.x % rg::kWave;
  const long row = (long)blockIdx.x * kWavesPerBlock + threadIdx.x / rg::kWave;      // p * h + y
  if (row >= rows) return;                                                           // the whole wavefront
  const long p = row / h, y = row - p * h;
  const size_t in_row = (size_t)row * (size_t)w, layer = (size_t)h * (size_t)w;
  const size_t out_row = (size_t)p * (size_t)n_thr * layer + (size_t)y * (size_t)w;
  const unsigned long long below = lanes_up_to(lane);
  int carry[RG_MAX_VERIFY_THRESHOLDS];
#pragma unroll
  for (int t = 0; t < RG_MAX_VERIFY_THRESHOLDS; ++t) carry[t] = 0;
  for (int x0 = 0; x0 < w; x0 += rg::kWave) {
    const int x = x0 + lane;
    const bool in = x < w;
    float v = 0.0f;
    bool ok = in;
    if (in) {
      v = src[in_row + x];
      ok = !isnan(v) && !(partner && isnan(partner[in_row + x])) && !(mask && mask[in_row + x]);
    }
#pragma unroll
    for (int t = 0; t < RG_MAX_VERIFY_THRESHOLDS; ++t) {
      if (t < n_thr) {
        const unsigned long long hit = __ballot(ok && v >= thr.t[t]);
        if (in) sat[out_row + (size_t)t * layer + x] = carry[t] + __builtin_popcountll(hit & below);
        carry[t] += __builtin_popcountll(hit);
      }
    }
  }
}

// ---- summed-area table: columns ----------------------------------------------------------------------------------------------
// blockIdx.y = the layer, one thread per column; the loads of kColumnUnroll rows do not wait for the running sum
__global__ __launch_bounds__(rg::kWave) void sat_columns_kernel(int* sat, int h, int w) {
  const int x = (int)(blockIdx.x * rg::kWave + threadIdx.x);
  if (x >= w) return;
  int* col = sat + (size_t)blockIdx.y * (size_t)h * (size_t)w + x;
  int run = 0, y = 0;
  for (; y + kColumnUnroll <= h; y += kColumnUnroll) {
    int v[kColumnUnroll];
#pragma unroll
    for (int k = 0; k < kColumnUnroll; ++k) v[k] = col[(size_t)(y + k) * w];
#pragma unroll
    for (int k = 0; k < kColumnUnroll; ++k) {
      run += v[k];
      col[(size_t)(y + k) * w] = run;
    }
  }
  for (; y < h; ++y) {
    run += col[(size_t)y * w];
    col[(size_t)y * w] = run;
  }
}

// ---- window counts -----------------------------------------------------------------------------------------------------------
// the exceedances inside the window of scale n at (y, x), cut to the plane: four corners of the inclusive table, a corner at
// index -1 contributing 0.  y1 >= y >= 0 and x1 >= x >= 0 for every n >= 1, so the far corner always lies in the plane.
__device__ __forceinline__ int window_count(const int* __restrict__ sat, int h, int w, int y, int x, int n) {
  const int half = n >> 1;
  const int ya = max(y - half, 0) - 1, yb = min(y - half + n - 1, h - 1);
  const int xa = max(x - half, 0) - 1, xb = min(x - half + n - 1, w - 1);
  int count = sat[(size_t)yb * w + xb];
  if (ya >= 0) count -= sat[(size_t)ya * w + xb];
  if (xa >= 0) count -= sat[(size_t)yb * w + xa];
  if (ya >= 0 && xa >= 0) count += sat[(size_t)ya * w + xa];
  return count;
}

// blockIdx = (strip, layer, scale); layer0 is the first layer of this launch
__global__ __launch_bounds__(rg::kBlock) void fss_sums_kernel(const int* __restrict__ sat_f, const int* __restrict__ sat_o,
                                                              long layer0, int h, int w, Scales scales, int n_scales,
                                                              long long* sums) {
  __shared__ unsigned long long part[kWavesPerBlock][3];
  const int lane = threadIdx.x % rg::kWave, wave = threadIdx.x / rg::kWave;
  const size_t layer = (size_t)layer0 + blockIdx.y;
  const int hw = h * w, n = scales.n[blockIdx.z];
  const int* f = sat_f + layer * (size_t)hw;
  const int* o = sat_o + layer * (size_t)hw;
  unsigned long long a = 0, b = 0, c = 0;
  const long step = (long)gridDim.x * rg::kBlock;
  for (long i = (long)blockIdx.x * rg::kBlock + threadIdx.x; i < hw; i += step) {
    const int y = (int)i / w, x = (int)i - y * w;
    const long long cf = window_count(f, h, w, y, x, n), co = window_count(o, h, w, y, x, n);
    a += (unsigned long long)((cf - co) * (cf - co));
    b += (unsigned long long)(cf * cf);
    c += (unsigned long long)(co * co);
  }
#pragma unroll
  for (int d = rg::kWave / 2; d > 0; d >>= 1) {
    a += __shfl_down(a, d);
    b += __shfl_down(b, d);
    c += __shfl_down(c, d);
  }
  if (lane == 0) {
    part[wave][0] = a;
    part[wave][1] = b;
    part[wave][2] = c;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long total = 0;
#pragma unroll
    for (int v = 0; v < kWavesPerBlock; ++v) total += part[v][threadIdx.x];
    if (total)
      __hip_atomic_fetch_add(sums + (layer * (size_t)n_scales + blockIdx.z) * 3 + threadIdx.x, (long long)total, RG_VER_RELAXED);
  }
}

__global__ __launch_bounds__(rg::kBlock) void box_fraction_kernel(const int* __restrict__ sat, long total, int h, int w, int n,
                                                                  double area, float* __restrict__ out) {
  const long i = (long)blockIdx.x * rg::kBlock + threadIdx.x;
  if (i >= total) return;
  const int hw = h * w;
  const long layer = i / hw;
  const int pixel = (int)(i - layer * hw), y = pixel / w, x = pixel - y * w;
  out[i] = (float)((double)window_count(sat + (size_t)layer * hw, h, w, y, x, n) / area);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
// 1 <= count, h and w not negative, h * w < 2^31
int check_shape(const char* who, const char* what, int64_t count, int32_t h, int32_t w) {
  RG_REQUIRE(count >= 1, RG_EINVAL, "%s: %s must be at least 1, got %lld", who, what, (long long)count);
  RG_REQUIRE(h >= 0 && w >= 0, RG_EINVAL, "%s: negative size %d x %d", who, h, w);
  RG_REQUIRE((int64_t)h * w < ((int64_t)1 << 31), RG_EINVAL, "%s: h * w must stay below 2^31, got %d x %d", who, h, w);
  return RG_OK;
}

int read_thresholds(const char* who, const float* thresholds, int32_t n_thr, Thresholds* out) {
  RG_REQUIRE(n_thr >= 1 && n_thr <= RG_MAX_VERIFY_THRESHOLDS, RG_EINVAL, "%s: n_thr must lie in 1 .. %d, got %d", who,
             RG_MAX_VERIFY_THRESHOLDS, n_thr);
  for (int t = 0; t < RG_MAX_VERIFY_THRESHOLDS; ++t) {
    out->t[t] = t < n_thr ? thresholds[t] : NAN;
    RG_REQUIRE(t >= n_thr || isfinite(out->t[t]), RG_EINVAL, "%s: threshold %d is not finite", who, t);
  }
  return RG_OK;
}

inline bool scale_ok(int32_t n) { return n >= 1 && n <= RG_MAX_VERIFY_SCALE; }

inline unsigned strips_for(int64_t hw) { return (unsigned)std::min<int64_t>((hw + rg::kBlock - 1) / rg::kBlock, kMaxStrips); }

}  // namespace

extern "C" int rg_contingency_f32(const float* fcst, const float* obs, const uint8_t* mask, int32_t n_planes, int32_t h, int32_t w,
                                  const float* thresholds_host, int32_t n_thr, int64_t* counts, int64_t* valid,
                                  rg_stream_t stream) {
  const char* who = "rg_contingency_f32";
  RG_REQUIRE(fcst && obs && thresholds_host && counts && valid, RG_EINVAL, "%s: null pointer", who);
  int status = check_shape(who, "n_planes", n_planes, h, w);
  if (status != RG_OK) return status;
  RG_REQUIRE(n_planes <= 65535, RG_EINVAL, "%s: at most 65535 planes per call, got %d", who, n_planes);
  Thresholds thr;
  status = read_thresholds(who, thresholds_host, n_thr, &thr);
  if (status != RG_OK) return status;
  const int64_t hw = (int64_t)h * w, in_bytes = n_planes * hw * 4, count_bytes = (int64_t)n_planes * n_thr * 24;
  RG_REQUIRE(!rg::overlap(counts, count_bytes, valid, (int64_t)n_planes * 8), RG_EINVAL, "%s: counts overlaps valid", who);
  RG_REQUIRE(!rg::overlap(fcst, in_bytes, counts, count_bytes) && !rg::overlap(fcst, in_bytes, valid, (int64_t)n_planes * 8) &&
                 !rg::overlap(obs, in_bytes, counts, count_bytes) && !rg::overlap(obs, in_bytes, valid, (int64_t)n_planes * 8),
             RG_EINVAL, "%s: an output overlaps an input", who);
  const hipStream_t s = (hipStream_t)stream;
  rg::fill_words(counts, count_bytes, 0u, s);
  rg::fill_words(valid, (int64_t)n_planes * 8, 0u, s);
  if (hw == 0) return rg::check_launch(who);
  hipLaunchKernelGGL(contingency_kernel, dim3(strips_for(hw), (unsigned)n_planes), dim3(rg::kBlock), 0, s, fcst, obs, mask, (int)hw,
                     thr, n_thr, reinterpret_cast<long long*>(counts), reinterpret_cast<long long*>(valid));
  return rg::check_launch(who);
}

extern "C" int rg_exceedance_sat_i32(const float* src, const float* partner, const uint8_t* mask, int32_t n_planes, int32_t h,
                                     int32_t w, const float* thresholds_host, int32_t n_thr, int32_t* sat, rg_stream_t stream) {
  const char* who = "rg_exceedance_sat_i32";
  RG_REQUIRE(src && thresholds_host && sat, RG_EINVAL, "%s: null pointer", who);
  int status = check_shape(who, "n_planes", n_planes, h, w);
  if (status != RG_OK) return status;
  Thresholds thr;
  status = read_thresholds(who, thresholds_host, n_thr, &thr);
  if (status != RG_OK) return status;
  const int64_t hw = (int64_t)h * w, rows = (int64_t)n_planes * h, layers = (int64_t)n_planes * n_thr;
  RG_REQUIRE(layers <= 65535, RG_EINVAL, "%s: at most 65535 layers (n_planes * n_thr) per call, got %lld", who, (long long)layers);
  RG_REQUIRE(!rg::overlap(src, n_planes * hw * 4, sat, layers * hw * 4) &&
                 !(partner && rg::overlap(partner, n_planes * hw * 4, sat, layers * hw * 4)) &&
                 !(mask && rg::overlap(mask, n_planes * hw, sat, layers * hw * 4)),
             RG_EINVAL, "%s: sat overlaps an input", who);
  if (hw == 0) return RG_OK;
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sat_rows_kernel, dim3((unsigned)((rows + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(rg::kBlock), 0, s, src,
                     partner, mask, (long)rows, h, w, thr, n_thr, sat);
  hipLaunchKernelGGL(sat_columns_kernel, dim3((unsigned)((w + rg::kWave - 1) / rg::kWave), (unsigned)layers), dim3(rg::kWave), 0, s,
                     sat, h, w);
  return rg::check_launch(who);
}

extern "C" int rg_fss_sums_i32(const int32_t* sat_f, const int32_t* sat_o, int32_t n_layers, int32_t h, int32_t w,
                               const int32_t* scales_host, int32_t n_scales, int64_t* sums, rg_stream_t stream) {
  const char* who = "rg_fss_sums_i32";
  RG_REQUIRE(sat_f && sat_o && scales_host && sums, RG_EINVAL, "%s: null pointer", who);
  const int status = check_shape(who, "n_layers", n_layers, h, w);
  if (status != RG_OK) return status;
  RG_REQUIRE(n_scales >= 1 && n_scales <= RG_MAX_VERIFY_SCALES, RG_EINVAL, "%s: n_scales must lie in 1 .. %d, got %d", who,
             RG_MAX_VERIFY_SCALES, n_scales);
  const int64_t hw = (int64_t)h * w;
  Scales scales = {};
  for (int k = 0; k < n_scales; ++k) {
    scales.n[k] = scales_host[k];
    RG_REQUIRE(scale_ok(scales.n[k]), RG_EINVAL, "%s: scale %d must lie in 1 .. %d, got %d", who, k, RG_MAX_VERIFY_SCALE, scales.n[k]);
    // the largest window count is min(n^2, h * w); its square summed over h * w pixels must fit the int64 sum
    const __int128 most = std::min<int64_t>((int64_t)scales.n[k] * scales.n[k], hw);
    RG_REQUIRE(most * most * hw < ((__int128)1 << 63), RG_EINVAL, "%s: scale %d on %d x %d pixels can overflow the 64-bit sums", who,
               scales.n[k], h, w);
  }
  const int64_t sat_bytes = n_layers * hw * 4, sum_bytes = (int64_t)n_layers * n_scales * 24;
  RG_REQUIRE(!rg::overlap(sat_f, sat_bytes, sums, sum_bytes) && !rg::overlap(sat_o, sat_bytes, sums, sum_bytes), RG_EINVAL,
             "%s: sums overlaps an input", who);
  const hipStream_t s = (hipStream_t)stream;
  rg::fill_words(sums, sum_bytes, 0u, s);
  if (hw == 0) return rg::check_launch(who);
  for (int64_t layer0 = 0; layer0 < n_layers; layer0 += kLayersPerLaunch) {
    const unsigned layers = (unsigned)std::min<int64_t>(n_layers - layer0, kLayersPerLaunch);
    hipLaunchKernelGGL(fss_sums_kernel, dim3(strips_for(hw), layers, (unsigned)n_scales), dim3(rg::kBlock), 0, s, sat_f, sat_o,
                       (long)layer0, h, w, scales, n_scales, reinterpret_cast<long long*>(sums));
  }
  return rg::check_launch(who);
}

extern "C" int rg_box_fraction_f32(const int32_t* sat, int32_t n_layers, int32_t h, int32_t w, int32_t scale, float* out,
                                   rg_stream_t stream) {
  const char* who = "rg_box_fraction_f32";
  RG_REQUIRE(sat && out, RG_EINVAL, "%s: null pointer", who);
  const int status = check_shape(who, "n_layers", n_layers, h, w);
  if (status != RG_OK) return status;
  RG_REQUIRE(scale_ok(scale), RG_EINVAL, "%s: scale must lie in 1 .. %d, got %d", who, RG_MAX_VERIFY_SCALE, scale);
  const int64_t total = (int64_t)n_layers * h * w;
  RG_REQUIRE(total < ((int64_t)1 << 40), RG_EINVAL, "%s: n_layers * h * w must stay below 2^40", who);
  RG_REQUIRE(!rg::overlap(sat, total * 4, out, total * 4), RG_EINVAL, "%s: out overlaps sat", who);
  if (total == 0) return RG_OK;
  hipLaunchKernelGGL(box_fraction_kernel, dim3((unsigned)((total + rg::kBlock - 1) / rg::kBlock)), dim3(rg::kBlock), 0,
                     (hipStream_t)stream, sat, (long)total, h, w, scale, (double)(scale * scale), out);
  return rg::check_launch(who);
}
