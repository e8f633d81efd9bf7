// Convective / stratiform classification after Steiner, Houze and Yuter 1995 (include/radargrid_hip.h, "Convective /
// stratiform classification"): the background reflectivity as a disk mean of LINEAR reflectivity, the convective centres, and
// the convective area as a dilation whose radius depends on the centre's class.
//
// Reflectivity is summed in 2^-16 fixed point, so every sum is an integer: a disk sum is a sum of differences of row prefixes
// (csrc/rg_disk.hpp), exact modulo 2^64 whatever the order, and every output is bit-reproducible.
//   echo table    one wavefront per row, 64 pixels per trip: q = llrint(65536 * exp10(dBZ / 10)) per echo pixel, a shuffle
//                 ladder for the 64-bit prefix, one ballot for the echo count; the carries cross the trips in scalar registers.
//                 One 16-byte entry {prefix of q, prefix of the count} per pixel, w + 1 per row.
//   background    one wavefront per 64 pixels of a row, four rows per workgroup: two entry loads per covered row, the row
//                 distance and the half-width wave-uniform; one float64 division and log10 per pixel
//   centres       one thread per pixel, float64 comparisons
//   area          per class, the row prefixes of "is a centre of this class" (one ballot per class and trip), then per echo
//                 pixel the footprint count of every class through the same disk_sum, stopping at the first hit
#include <math.h>

#include <algorithm>

#include "rg_disk.hpp"

namespace {

constexpr int kWavesPerBlock = rg::kBlock / rg::kWave;     // rows of a workgroup's tile
constexpr int kMaxPlanes = 65535;                          // gridDim.y

// {prefix of q, prefix of the echo count}: one load serves both
struct alignas(16) EchoEntry {
  unsigned long long s;
  uint32_t c;
  uint32_t reserved;
  struct Sum {
    unsigned long long s;
    uint32_t c;
    __device__ __forceinline__ void add(const EchoEntry& hi, const EchoEntry& lo) {
      s += hi.s - lo.s;
      c += hi.c - lo.c;
    }
  };
};
static_assert(sizeof(EchoEntry) == 16, "the echo table is one 16-byte entry per pixel");

struct Edges {
  double e[RG_MAX_CONV_CLASSES - 1];      // entries from n_classes - 1 on are +inf, which no background reaches
};

struct Footprints {
  rg::Footprint f[RG_MAX_CONV_CLASSES];
};

__device__ __forceinline__ unsigned long long lanes_up_to(int lane) { return ~0ull >> (63 - lane); }

__device__ __forceinline__ bool has_echo(float v, const uint8_t* __restrict__ mask, size_t i, float min_dbz) {
  return !isnan(v) && !(mask && mask[i]) && v >= min_dbz;
}

// the tile of a workgroup: 64 pixels of kWavesPerBlock rows; blockIdx.x = ty * tiles_x + tx, blockIdx.y = the plane.
// y is wave-uniform by construction and made so for the compiler.
__device__ __forceinline__ void tile_pixel(int tiles_x, int* y, int* x) {
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / rg::kWave), lane = threadIdx.x % rg::kWave;
  const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
  *y = ty * kWavesPerBlock + wave;
  *x = tx * rg::kWave + lane;
}

// ---- echo table --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(rg::kBlock) void echo_rows_kernel(const float* __restrict__ dbz, const uint8_t* __restrict__ mask,
                                                               long rows, int w, float min_dbz, EchoEntry* __restrict__ table) {
  const int lane = threadIdx.x % rg::kWave;
  const long row = (long)blockIdx.x * kWavesPerBlock + threadIdx.x / rg::kWave;      // p * h + y
  if (row >= rows) return;                                                           // the whole wavefront
  const size_t in_row = (size_t)row * (size_t)w;
  EchoEntry* out = table + (size_t)row * rg::prefix_pitch(w);
  if (lane == 0) out[0] = EchoEntry{0ull, 0u, 0u};
  const unsigned long long below = lanes_up_to(lane);
  unsigned long long carry_s = 0;
  uint32_t carry_c = 0;
  for (long x0 = 0; x0 < w; x0 += rg::kWave) {
    const long x = x0 + lane;
    const bool in = x < w;
    unsigned long long s = 0;
    bool echo = false;
    if (in) {
      const float v = dbz[in_row + x];
      echo = has_echo(v, mask, in_row + x, min_dbz);
      if (echo) s = (unsigned long long)llrint(65536.0 * exp10(fmin(fmax((double)v, -10.0), 80.0) / 10.0));
    }
    const unsigned long long hit = __ballot(echo);
#pragma unroll
    for (int d = 1; d < rg::kWave; d <<= 1) {
      const unsigned long long t = __shfl_up(s, d);
      if (lane >= d) s += t;
    }
    if (in) out[x + 1] = EchoEntry{carry_s + s, carry_c + (uint32_t)__builtin_popcountll(hit & below), 0u};
    carry_s += __shfl(s, rg::kWave - 1);
    carry_c += (uint32_t)__builtin_popcountll(hit);
  }
}

// ---- disk background ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(rg::kBlock) void disk_background_kernel(const EchoEntry* __restrict__ table, int h, int w, int tiles_x,
                                                                     rg::Footprint fp, long long* __restrict__ out_sum,
                                                                     int* __restrict__ out_count, float* __restrict__ out_bkg) {
  int y, x;
  tile_pixel(tiles_x, &y, &x);
  if (y >= h || x >= w) return;
  const size_t plane = blockIdx.y;
  const EchoEntry::Sum sum = rg::disk_sum<4>(table + plane * (size_t)h * rg::prefix_pitch(w), h, w, y, x, fp);
  const size_t i = (plane * (size_t)h + (size_t)y) * (size_t)w + (size_t)x;
  if (out_sum) out_sum[i] = (long long)sum.s;
  if (out_count) out_count[i] = (int)sum.c;
  if (out_bkg) out_bkg[i] = sum.c ? (float)(10.0 * log10((double)(long long)sum.s / (double)sum.c / 65536.0)) : NAN;
}

// ---- convective centres ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(rg::kBlock) void centres_kernel(const float* __restrict__ dbz, const uint8_t* __restrict__ mask,
                                                             const float* __restrict__ bkg, long total, float min_dbz, double intense,
                                                             double peak_a, double peak_b, Edges edges, uint8_t* __restrict__ out) {
  const long i = (long)blockIdx.x * rg::kBlock + threadIdx.x;
  if (i >= total) return;
  const float vf = dbz[i];
  uint8_t k = 0;
  if (has_echo(vf, mask, (size_t)i, min_dbz)) {
    const double v = (double)vf, b = (double)bkg[i];
    const double curve = peak_a - b * b / peak_b;
    const double delta = b < 0.0 ? peak_a : (curve > 0.0 ? curve : 0.0);
    if (v >= intense || (v - b) >= delta) {
      k = 1;
#pragma unroll
      for (int e = 0; e < RG_MAX_CONV_CLASSES - 1; ++e) k += b >= edges.e[e] ? 1 : 0;
    }
  }
  out[i] = k;
}

// ---- convective area ---------------------------------------------------------------------------------------------------------
// one wavefront per row: counts[k][row][x + 1] = the centres of class k + 1 in columns 0 .. x of the row
__global__ __launch_bounds__(rg::kBlock) void centre_rows_kernel(const uint8_t* __restrict__ centres, long rows, int w, int n_classes,
                                                                 rg::CountEntry* __restrict__ counts) {
  const int lane = threadIdx.x % rg::kWave;
  const long row = (long)blockIdx.x * kWavesPerBlock + threadIdx.x / rg::kWave;
  if (row >= rows) return;
  const size_t in_row = (size_t)row * (size_t)w, pitch = rg::prefix_pitch(w), layer = (size_t)rows * pitch;
  rg::CountEntry* out = counts + (size_t)row * pitch;
  if (lane < n_classes) out[(size_t)lane * layer].c = 0;
  const unsigned long long below = lanes_up_to(lane);
  int carry[RG_MAX_CONV_CLASSES];
#pragma unroll
  for (int k = 0; k < RG_MAX_CONV_CLASSES; ++k) carry[k] = 0;
  for (long x0 = 0; x0 < w; x0 += rg::kWave) {
    const long x = x0 + lane;
    const bool in = x < w;
    const int c = in ? centres[in_row + x] : 0;
#pragma unroll
    for (int k = 0; k < RG_MAX_CONV_CLASSES; ++k) {
      if (k < n_classes) {
        const unsigned long long hit = __ballot(c == k + 1);
        if (in) out[(size_t)k * layer + x + 1].c = carry[k] + __builtin_popcountll(hit & below);
        carry[k] += __builtin_popcountll(hit);
      }
    }
  }
}

__global__ __launch_bounds__(rg::kBlock) void area_kernel(const rg::CountEntry* __restrict__ counts, const float* __restrict__ dbz,
                                                          const uint8_t* __restrict__ mask, int n, int h, int w, int tiles_x,
                                                          float min_dbz, int n_classes, Footprints fps, uint8_t* __restrict__ out) {
  int y, x;
  tile_pixel(tiles_x, &y, &x);
  if (y >= h || x >= w) return;
  const size_t plane = blockIdx.y, pitch = rg::prefix_pitch(w);
  const size_t i = (plane * (size_t)h + (size_t)y) * (size_t)w + (size_t)x;
  uint8_t cls = 0;
  if (has_echo(dbz[i], mask, i, min_dbz)) {
    cls = 1;
    for (int k = 0; k < n_classes; ++k) {            // at most RG_MAX_CONV_CLASSES trips
      if (cls == 1) {
        const rg::CountEntry* table = counts + ((size_t)k * (size_t)n + plane) * (size_t)h * pitch;
        // both loops rolled: with the row loop unrolled the compiler expands the nest to 1 500 loads and 170 VGPRs
        if (rg::disk_sum<1>(table, h, w, y, x, fps.f[k]).c > 0) cls = 2;
      }
    }
  }
  out[i] = cls;
}

// ---- host --------------------------------------------------------------------------------------------------------------------
// 1 <= n <= 65535, h and w not negative, h * w < 2^31
int check_shape(const char* who, int64_t n, int32_t h, int32_t w) {
  RG_REQUIRE(n >= 1 && n <= kMaxPlanes, RG_EINVAL, "%s: n must lie in 1 .. %d, got %lld", who, kMaxPlanes, (long long)n);
  RG_REQUIRE(h >= 0 && w >= 0, RG_EINVAL, "%s: negative size %d x %d", who, h, w);
  RG_REQUIRE((int64_t)h * w < ((int64_t)1 << 31), RG_EINVAL, "%s: h * w must stay below 2^31, got %d x %d", who, h, w);
  return RG_OK;
}

inline int64_t prefix_entries(int64_t n, int32_t h, int32_t w) { return n * h * ((int64_t)w + 1); }

inline int tiles_x_for(int32_t w) { return (w + rg::kWave - 1) / rg::kWave; }

// the tiles of one plane; below 2^31 whenever h * w is
inline unsigned tiles_for(int32_t h, int32_t w) { return (unsigned)((int64_t)tiles_x_for(w) * ((h + kWavesPerBlock - 1) / kWavesPerBlock)); }

inline unsigned row_blocks(int64_t rows) { return (unsigned)((rows + kWavesPerBlock - 1) / kWavesPerBlock); }

}  // namespace

extern "C" int64_t rg_echo_table_bytes(int32_t n, int32_t h, int32_t w) {
  const int status = check_shape("rg_echo_table_bytes", n, h, w);
  if (status != RG_OK) return status;
  return h == 0 || w == 0 ? 0 : prefix_entries(n, h, w) * (int64_t)sizeof(EchoEntry);
}

extern "C" int rg_echo_table_f32(const float* dbz, const uint8_t* mask, int32_t n, int32_t h, int32_t w, float min_dbz, void* table,
                                 int64_t table_bytes, rg_stream_t stream) {
  const char* who = "rg_echo_table_f32";
  RG_REQUIRE(dbz && table, RG_EINVAL, "%s: null pointer", who);
  const int status = check_shape(who, n, h, w);
  if (status != RG_OK) return status;
  RG_REQUIRE(isfinite(min_dbz), RG_EINVAL, "%s: min_dbz is not finite", who);
  const int64_t hw = (int64_t)h * w, need = hw ? prefix_entries(n, h, w) * (int64_t)sizeof(EchoEntry) : 0;
  RG_REQUIRE(table_bytes >= need, RG_EWORKSPACE, "%s: the table needs %lld bytes, got %lld", who, (long long)need,
             (long long)table_bytes);
  RG_REQUIRE(rg::aligned16(table), RG_EALIGN, "%s: the table must be 16-byte aligned", who);
  RG_REQUIRE(!rg::overlap(dbz, n * hw * 4, table, need) && !(mask && rg::overlap(mask, n * hw, table, need)), RG_EINVAL,
             "%s: the table overlaps an input", who);
  if (hw == 0) return RG_OK;
  const int64_t rows = (int64_t)n * h;
  hipLaunchKernelGGL(echo_rows_kernel, dim3(row_blocks(rows)), dim3(rg::kBlock), 0, (hipStream_t)stream, dbz, mask, (long)rows, w,
                     min_dbz, static_cast<EchoEntry*>(table));
  return rg::check_launch(who);
}

extern "C" int rg_disk_background(const void* table, int32_t n, int32_t h, int32_t w, const int32_t* hw_host, int32_t ry,
                                  int64_t* out_sum, int32_t* out_count, float* out_bkg, rg_stream_t stream) {
  const char* who = "rg_disk_background";
  RG_REQUIRE(table && hw_host, RG_EINVAL, "%s: null pointer", who);
  RG_REQUIRE(out_sum || out_count || out_bkg, RG_EINVAL, "%s: at least one output must be given", who);
  int status = check_shape(who, n, h, w);
  if (status != RG_OK) return status;
  rg::Footprint fp;
  status = rg::read_footprint(who, hw_host, ry, &fp);
  if (status != RG_OK) return status;
  RG_REQUIRE(rg::aligned16(table), RG_EALIGN, "%s: the table must be 16-byte aligned", who);
  const int64_t hw = (int64_t)h * w, pixels = n * hw, table_bytes = hw ? prefix_entries(n, h, w) * (int64_t)sizeof(EchoEntry) : 0;
  const void* outs[] = {out_sum, out_count, out_bkg};
  const int64_t widths[] = {8, 4, 4};
  for (int a = 0; a < 3; ++a) {
    if (!outs[a]) continue;
    RG_REQUIRE(!rg::overlap(table, table_bytes, outs[a], pixels * widths[a]), RG_EINVAL, "%s: an output overlaps the table", who);
    for (int b = a + 1; b < 3; ++b)
      RG_REQUIRE(!outs[b] || !rg::overlap(outs[a], pixels * widths[a], outs[b], pixels * widths[b]), RG_EINVAL,
                 "%s: two outputs overlap", who);
  }
  if (hw == 0) return RG_OK;
  hipLaunchKernelGGL(disk_background_kernel, dim3(tiles_for(h, w), (unsigned)n), dim3(rg::kBlock), 0, (hipStream_t)stream,
                     static_cast<const EchoEntry*>(table), h, w, tiles_x_for(w), fp, reinterpret_cast<long long*>(out_sum), out_count,
                     out_bkg);
  return rg::check_launch(who);
}

extern "C" int rg_convective_centres_f32(const float* dbz, const uint8_t* mask, const float* bkg, int32_t n, int32_t h, int32_t w,
                                         float min_dbz, double intense, double peak_a, double peak_b, const double* edges_host,
                                         int32_t n_classes, uint8_t* out_class, rg_stream_t stream) {
  const char* who = "rg_convective_centres_f32";
  RG_REQUIRE(dbz && bkg && out_class, RG_EINVAL, "%s: null pointer", who);
  const int status = check_shape(who, n, h, w);
  if (status != RG_OK) return status;
  RG_REQUIRE(n_classes >= 1 && n_classes <= RG_MAX_CONV_CLASSES, RG_EINVAL, "%s: n_classes must lie in 1 .. %d, got %d", who,
             RG_MAX_CONV_CLASSES, n_classes);
  RG_REQUIRE(n_classes == 1 || edges_host, RG_EINVAL, "%s: null edges for %d classes", who, n_classes);
  RG_REQUIRE(isfinite(min_dbz) && isfinite(intense) && isfinite(peak_a) && isfinite(peak_b), RG_EINVAL,
             "%s: min_dbz, intense, peak_a and peak_b must be finite", who);
  RG_REQUIRE(peak_b > 0.0, RG_EINVAL, "%s: peak_b must be positive, got %g", who, peak_b);
  Edges edges;
  for (int e = 0; e < RG_MAX_CONV_CLASSES - 1; ++e) {
    edges.e[e] = e < n_classes - 1 ? edges_host[e] : (double)INFINITY;
    RG_REQUIRE(e >= n_classes - 1 || isfinite(edges.e[e]), RG_EINVAL, "%s: edge %d is not finite", who, e);
    RG_REQUIRE(e == 0 || e >= n_classes - 1 || edges.e[e] >= edges.e[e - 1], RG_EINVAL, "%s: edge %d descends", who, e);
  }
  const int64_t total = (int64_t)n * h * w;
  RG_REQUIRE(!rg::overlap(dbz, total * 4, out_class, total) && !rg::overlap(bkg, total * 4, out_class, total) &&
                 !(mask && rg::overlap(mask, total, out_class, total)),
             RG_EINVAL, "%s: out_class overlaps an input", who);
  if (total == 0) return RG_OK;
  hipLaunchKernelGGL(centres_kernel, dim3((unsigned)((total + rg::kBlock - 1) / rg::kBlock)), dim3(rg::kBlock), 0,
                     (hipStream_t)stream, dbz, mask, bkg, (long)total, min_dbz, intense, peak_a, peak_b, edges, out_class);
  return rg::check_launch(who);
}

extern "C" int64_t rg_convective_area_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t n_classes) {
  const char* who = "rg_convective_area_workspace_bytes";
  const int status = check_shape(who, n, h, w);
  if (status != RG_OK) return status;
  RG_REQUIRE(n_classes >= 1 && n_classes <= RG_MAX_CONV_CLASSES, RG_EINVAL, "%s: n_classes must lie in 1 .. %d, got %d", who,
             RG_MAX_CONV_CLASSES, n_classes);
  return h == 0 || w == 0 ? 0 : prefix_entries(n, h, w) * n_classes * (int64_t)sizeof(rg::CountEntry);
}

extern "C" int rg_convective_area_u8(const uint8_t* centres, const float* dbz, const uint8_t* mask, int32_t n, int32_t h, int32_t w,
                                     float min_dbz, int32_t n_classes, const int32_t* hw_host, const int32_t* ry_host, void* workspace,
                                     int64_t workspace_bytes, uint8_t* out, rg_stream_t stream) {
  const char* who = "rg_convective_area_u8";
  RG_REQUIRE(centres && dbz && hw_host && ry_host && out, RG_EINVAL, "%s: null pointer", who);
  int status = check_shape(who, n, h, w);
  if (status != RG_OK) return status;
  RG_REQUIRE(n_classes >= 1 && n_classes <= RG_MAX_CONV_CLASSES, RG_EINVAL, "%s: n_classes must lie in 1 .. %d, got %d", who,
             RG_MAX_CONV_CLASSES, n_classes);
  RG_REQUIRE(isfinite(min_dbz), RG_EINVAL, "%s: min_dbz is not finite", who);
  Footprints fps = {};
  for (int k = 0; k < n_classes; ++k) {
    status = rg::read_footprint(who, hw_host + (size_t)k * (RG_MAX_DISK_RADIUS + 1), ry_host[k], &fps.f[k]);
    if (status != RG_OK) return status;
  }
  const int64_t hw = (int64_t)h * w, total = n * hw;
  const int64_t need = hw ? prefix_entries(n, h, w) * n_classes * (int64_t)sizeof(rg::CountEntry) : 0;
  RG_REQUIRE(workspace_bytes >= need, RG_EWORKSPACE, "%s: the workspace needs %lld bytes, got %lld", who, (long long)need,
             (long long)workspace_bytes);
  RG_REQUIRE(need == 0 || (workspace && (reinterpret_cast<uintptr_t>(workspace) & 3u) == 0), RG_EINVAL,
             "%s: the workspace is null or not 4-byte aligned", who);
  RG_REQUIRE(!rg::overlap(centres, total, out, total) && !rg::overlap(dbz, total * 4, out, total) &&
                 !(mask && rg::overlap(mask, total, out, total)),
             RG_EINVAL, "%s: out overlaps an input", who);
  RG_REQUIRE(need == 0 || (!rg::overlap(workspace, need, out, total) && !rg::overlap(workspace, need, centres, total) &&
                           !rg::overlap(workspace, need, dbz, total * 4) && !(mask && rg::overlap(workspace, need, mask, total))),
             RG_EINVAL, "%s: the workspace overlaps an operand", who);
  if (hw == 0) return RG_OK;
  const hipStream_t s = (hipStream_t)stream;
  const int64_t rows = (int64_t)n * h;
  rg::CountEntry* counts = static_cast<rg::CountEntry*>(workspace);
  hipLaunchKernelGGL(centre_rows_kernel, dim3(row_blocks(rows)), dim3(rg::kBlock), 0, s, centres, (long)rows, w, n_classes, counts);
  hipLaunchKernelGGL(area_kernel, dim3(tiles_for(h, w), (unsigned)n), dim3(rg::kBlock), 0, s, counts, dbz, mask, n, h, w,
                     tiles_x_for(w), min_dbz, n_classes, fps, out);
  return rg::check_launch(who);
}
