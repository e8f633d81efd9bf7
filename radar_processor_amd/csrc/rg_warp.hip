// Onto a web map (include/radargrid_hip.h, rg_mercator_raster / rg_warp_source): a product plane or its RGBA image
// resampled north-up into a Web Mercator raster, and the overview levels of such an image.
//
// The warp is float64 VALU work with a small gather, not a bandwidth problem.  Of the map's transcendentals, tanh / cosh
// depend only on the raster row and sincos only on the column, so a block evaluates them ONCE for the 32 rows and 64 columns
// of its tile into LDS (96 evaluations for 2 048 pixels); per pixel remain hypot, atan2, three divisions and a handful of
// multiplies.  (Measured: evaluating them per pixel instead takes 2.1x as long on a 2000 x 2000 plane, with the same bits:
// profiles/warp_timing.json, EXPERIMENTS.md.)  A wavefront is 64 consecutive pixels of one row: stores are coalesced along
// `width`, the gather touches a few neighbouring source rows.  Built with FP contraction off like every other unit: the steps
// are the header's, in its order.
#include <math.h>
#include <string.h>

#include "rg_common.hpp"
#include "rg_sample.hpp"

namespace {

constexpr double kMercatorRadius = 6378137.0;                       // the EPSG:3857 sphere
constexpr double kMaxAngularDistance = 3.14159265358979323846 / 2.0 - 0.1;
constexpr int kTileW = 64, kTileH = 32;                             // pixels of one block: 256 threads x 8 rows each
constexpr int kRowsPerPass = rg::kBlock / kTileW;
constexpr long kTilesPerLaunch = 1L << 23;                          // x 256 threads = 2^31 work-items (a dispatch holds < 2^32)
constexpr long kPerLaunch = 1L << 31;
enum { kNearest = 0, kBilinear = 1, kRgba = 2 };

__device__ __forceinline__ void column_terms(const rg_mercator_raster& m, const rg_georef& g, int c, double* sd, double* cd) {
  const double X = m.x_min + ((double)c + 0.5) * m.pixel;
  sincos(X / kMercatorRadius - g.lon_to, sd, cd);
}

__device__ __forceinline__ void row_terms(const rg_mercator_raster& m, int r, double* sp, double* cp) {
  const double t = (m.y_max - ((double)r + 0.5) * m.pixel) / kMercatorRadius;
  *sp = tanh(t);
  *cp = 1.0 / cosh(t);
}

// the header's AEQD forward map fed sines and cosines; false: the pixel lies beyond the angular limit
__device__ __forceinline__ bool plane_coords(const rg_georef& g, const rg_warp_source& s, double sp, double cp, double sd,
                                             double cd, double* fx, double* fy) {
  const double a = cp * sd;
  const double b = g.cos_lat_to * sp - g.sin_lat_to * cp * cd;
  const double q = g.sin_lat_to * sp + g.cos_lat_to * cp * cd;
  const double h = hypot(a, b);
  const double c = atan2(h, q);
  const double k = h == 0.0 ? 1.0 : c / h;
  *fx = (g.radius * k * a - s.x_lo) / s.step_x;
  *fy = (g.radius * k * b - s.y_lo) / s.step_y;
  return c < kMaxAngularDistance;
}

// MODE kNearest / kBilinear: float32 planes (moved as their bits where they are only copied); kRgba: one 32-bit pixel
template <int MODE>
__global__ __launch_bounds__(rg::kBlock) void warp_kernel(const uint32_t* __restrict__ src, int n_planes, rg_warp_source s,
                                                          rg_georef g, rg_mercator_raster m, uint32_t fill, long first_tile,
                                                          long tiles_x, uint32_t* __restrict__ out) {
  const long tile = first_tile + blockIdx.x;
  const long tile_row = tile / tiles_x;
  const int r0 = (int)tile_row * kTileH, c0 = (int)(tile - tile_row * tiles_x) * kTileW;
  const int lane_c = threadIdx.x % kTileW, lane_r = threadIdx.x / kTileW;
  __shared__ double col_sd[kTileW], col_cd[kTileW], row_sp[kTileH], row_cp[kTileH];
  if (threadIdx.x < kTileW)
    column_terms(m, g, c0 + threadIdx.x, &col_sd[threadIdx.x], &col_cd[threadIdx.x]);
  else if (threadIdx.x < kTileW + kTileH)
    row_terms(m, r0 + (threadIdx.x - kTileW), &row_sp[threadIdx.x - kTileW], &row_cp[threadIdx.x - kTileW]);
  __syncthreads();
  const double sd = col_sd[lane_c], cd = col_cd[lane_c];
  const int c = c0 + lane_c;
  if (c >= m.width) return;
  const size_t plane_in = (size_t)s.ny * s.nx, plane_out = (size_t)m.height * m.width;
  for (int j = lane_r; j < kTileH; j += kRowsPerPass) {
    const int r = r0 + j;
    if (r >= m.height) return;
    const double sp = row_sp[j], cp = row_cp[j];
    double fx, fy;
    const bool visible = plane_coords(g, s, sp, cp, sd, cd, &fx, &fy);
    uint32_t* o = out + (size_t)r * m.width + c;
    if constexpr (MODE == kBilinear) {
      const rg::BilinearTaps taps = rg::bilinear_taps(fx, fy, s.nx, s.ny, visible);
      for (int p = 0; p < n_planes; ++p) o[p * plane_out] = rg::bilinear_sample(src + p * plane_in, s.nx, taps, fill);
    } else {
      size_t at;
      const bool inside = rg::nearest_node(fx, fy, s.nx, s.ny, visible, &at);
      for (int p = 0; p < n_planes; ++p) o[p * plane_out] = inside ? src[p * plane_in + at] : fill;
    }
  }
}

__device__ __forceinline__ long lmin(long a, long b) { return a < b ? a : b; }

// one thread per output pixel of one overview level; src / out as bits where the value is only copied
template <bool AVERAGE>
__global__ __launch_bounds__(rg::kBlock) void overview_kernel(const uint32_t* __restrict__ src, int h, int w, int f, int oh,
                                                              int ow, long first, long n, uint32_t* __restrict__ out) {
  const long i = first + (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long row = i / ow;                        // over all planes
  const long p = row / oh;
  const long r = row - p * oh, c = i - row * ow;
  const uint32_t* plane = src + (size_t)p * h * w;
  if constexpr (AVERAGE) {
    const long y1 = lmin((r + 1) * f, h), x1 = lmin((c + 1) * f, w);
    double sum = 0.0;
    int count = 0;
    for (long y = r * f; y < y1; ++y)
      for (long x = c * f; x < x1; ++x) {
        const float v = rg::bits_f32(plane[y * w + x]);
        if (isfinite(v)) {
          sum += (double)v;
          ++count;
        }
      }
    out[i] = rg::f32_bits(count ? (float)(sum / (double)count) : __builtin_nanf(""));
  } else {
    out[i] = plane[lmin(r * f + f / 2, h - 1) * w + lmin(c * f + f / 2, w - 1)];
  }
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// every refusal the two warp entry points share (a plane element is 4 bytes: a float, or an RGBA pixel)
int check_warp(const char* who, const void* src, int n_planes, const rg_warp_source* source, const rg_georef* grid,
               const rg_mercator_raster* raster, const void* out) {
  RG_REQUIRE(src && source && grid && raster && out, RG_EINVAL, "%s: null pointer", who);
  RG_REQUIRE(n_planes >= 1, RG_EINVAL, "%s: n_planes must be at least 1", who);
  const rg_warp_source& s = *source;
  const rg_mercator_raster& m = *raster;
  RG_REQUIRE(isfinite(grid->radius) && grid->radius > 0.0, RG_EINVAL, "%s: radius must be finite and positive", who);
  RG_REQUIRE(rg::georef_finite(*grid), RG_EINVAL, "%s: a member of rg_georef is not finite", who);
  RG_REQUIRE(isfinite(s.x_lo) && isfinite(s.y_lo) && isfinite(s.step_x) && isfinite(s.step_y), RG_EINVAL,
             "%s: a member of rg_warp_source is not finite", who);
  RG_REQUIRE(s.step_x > 0.0 && s.step_y > 0.0, RG_EINVAL, "%s: step_x and step_y must be positive", who);
  RG_REQUIRE(s.ny >= 2 && s.nx >= 2, RG_EINVAL, "%s: ny and nx must be at least 2", who);
  RG_REQUIRE(isfinite(m.x_min) && isfinite(m.y_max) && isfinite(m.pixel), RG_EINVAL,
             "%s: a member of rg_mercator_raster is not finite", who);
  RG_REQUIRE(m.pixel > 0.0, RG_EINVAL, "%s: pixel must be positive", who);
  RG_REQUIRE(m.width >= 0 && m.height >= 0, RG_EINVAL, "%s: negative width or height", who);
  RG_REQUIRE(!rg::overlap(src, (int64_t)n_planes * s.ny * s.nx * 4, out, (int64_t)n_planes * m.height * m.width * 4), RG_EINVAL,
             "%s: out overlaps src", who);
  return RG_OK;
}

template <int MODE>
void launch_warp(const void* src, int n_planes, const rg_warp_source& s, const rg_georef& g, const rg_mercator_raster& m,
                 uint32_t fill, void* out, rg_stream_t stream) {
  const long tiles_x = ((long)m.width + kTileW - 1) / kTileW, tiles_y = ((long)m.height + kTileH - 1) / kTileH;
  const long tiles = tiles_x * tiles_y;
  for (long first = 0; first < tiles; first += kTilesPerLaunch) {
    const long n = tiles - first < kTilesPerLaunch ? tiles - first : kTilesPerLaunch;
    hipLaunchKernelGGL(warp_kernel<MODE>, dim3((unsigned)n), dim3(rg::kBlock), 0, (hipStream_t)stream,
                       static_cast<const uint32_t*>(src), n_planes, s, g, m, fill, first, tiles_x, static_cast<uint32_t*>(out));
  }
}

template <bool AVERAGE>
int launch_overview(const char* who, const void* src, int32_t n_planes, int32_t h, int32_t w, int32_t factor, void* out,
                    rg_stream_t stream) {
  RG_REQUIRE(src && out, RG_EINVAL, "%s: null pointer", who);
  RG_REQUIRE(n_planes >= 1, RG_EINVAL, "%s: n_planes must be at least 1", who);
  RG_REQUIRE(h >= 0 && w >= 0, RG_EINVAL, "%s: negative size", who);
  RG_REQUIRE(factor >= 2 && factor <= 64, RG_EINVAL, "%s: factor must lie in 2 .. 64", who);
  const int oh = (int)(((long)h + factor - 1) / factor), ow = (int)(((long)w + factor - 1) / factor);
  RG_REQUIRE(!rg::overlap(src, (int64_t)n_planes * h * w * 4, out, (int64_t)n_planes * oh * ow * 4), RG_EINVAL,
             "%s: out overlaps src", who);
  const long n = (long)n_planes * oh * ow;
  for (long first = 0; first < n; first += kPerLaunch) {
    const long m = n - first < kPerLaunch ? n - first : kPerLaunch;
    hipLaunchKernelGGL(overview_kernel<AVERAGE>, dim3((unsigned)((m + rg::kBlock - 1) / rg::kBlock)), dim3(rg::kBlock), 0,
                       (hipStream_t)stream, static_cast<const uint32_t*>(src), h, w, factor, oh, ow, first, first + m,
                       static_cast<uint32_t*>(out));
  }
  return n == 0 ? RG_OK : rg::check_launch(who);
}

}  // namespace

extern "C" int rg_warp_mercator_f32(const float* src, int32_t n_planes, const rg_warp_source* source, const rg_georef* grid,
                                    const rg_mercator_raster* raster, int32_t method, float fill, float* out,
                                    rg_stream_t stream) {
  const int status = check_warp("rg_warp_mercator_f32", src, n_planes, source, grid, raster, out);
  if (status != RG_OK) return status;
  RG_REQUIRE(method == kNearest || method == kBilinear, RG_EINVAL, "rg_warp_mercator_f32: unknown method %d", method);
  if (raster->width == 0 || raster->height == 0) return RG_OK;
  uint32_t fill_bits;
  memcpy(&fill_bits, &fill, sizeof fill_bits);
  if (method == kNearest)
    launch_warp<kNearest>(src, n_planes, *source, *grid, *raster, fill_bits, out, stream);
  else
    launch_warp<kBilinear>(src, n_planes, *source, *grid, *raster, fill_bits, out, stream);
  return rg::check_launch("rg_warp_mercator_f32");
}

extern "C" int rg_warp_mercator_rgba8(const uint8_t* src, const rg_warp_source* source, const rg_georef* grid,
                                      const rg_mercator_raster* raster, uint8_t* out, rg_stream_t stream) {
  const int status = check_warp("rg_warp_mercator_rgba8", src, 1, source, grid, raster, out);
  if (status != RG_OK) return status;
  RG_REQUIRE(aligned4(src) && aligned4(out), RG_EALIGN, "rg_warp_mercator_rgba8: src and out must be 4-byte aligned");
  if (raster->width == 0 || raster->height == 0) return RG_OK;
  launch_warp<kRgba>(src, 1, *source, *grid, *raster, 0u, out, stream);
  return rg::check_launch("rg_warp_mercator_rgba8");
}

extern "C" int rg_overview_f32(const float* src, int32_t n_planes, int32_t h, int32_t w, int32_t factor, int32_t method,
                               float* out, rg_stream_t stream) {
  RG_REQUIRE(method == 0 || method == 1, RG_EINVAL, "rg_overview_f32: unknown method %d", method);
  return method == 1 ? launch_overview<true>("rg_overview_f32", src, n_planes, h, w, factor, out, stream)
                     : launch_overview<false>("rg_overview_f32", src, n_planes, h, w, factor, out, stream);
}

extern "C" int rg_overview_rgba8(const uint8_t* src, int32_t h, int32_t w, int32_t factor, uint8_t* out, rg_stream_t stream) {
  RG_REQUIRE(!src || !out || (aligned4(src) && aligned4(out)), RG_EALIGN, "rg_overview_rgba8: src and out must be 4-byte aligned");
  return launch_overview<false>("rg_overview_rgba8", src, 1, h, w, factor, out, stream);
}
