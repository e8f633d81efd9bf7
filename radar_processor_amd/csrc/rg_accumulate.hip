// Rain rate and accumulation (include/radargrid_hip.h, rg_rain_rate_f32 / rg_accumulate_advected_f32): dBZ planes to mm/h
// under Z = a R^b, and the rainfall depth of the interval between two rate planes, summed along the echo's motion.
//
// The accumulation is the fusion of 2 * n_steps advections (rg_motion.hip) and their blend: one thread owns one pixel, walks
// the n_steps sub-instants, fetches the earlier plane moved forward and the later plane moved backward with the advection's
// own position and sampling code (rg_motion_field.hpp, rg_sample.hpp), and keeps the running sums of its planes in registers.
// Nothing but the finished plane is written.  V(p), the one lattice read that every position of a pixel shares, is evaluated
// once; with substeps == 1 it is the only one.  A workgroup covers a tile of kTileH x kTileW pixels so that the gathers of
// neighbouring lanes fall into the same few cache lines whichever way the echo moves.  Every step is a float64 operation
// rounded once, in the header's order: the outputs are bit-reproducible.
#include <math.h>
#include <string.h>

#include "rg_common.hpp"
#include "rg_motion_field.hpp"
#include "rg_sample.hpp"

namespace {

enum { kNearest = 0, kBilinear = 1 };
constexpr int kTileW = 32, kTileH = 8;           // kTileW * kTileH == rg::kBlock; a wavefront covers 2 rows of 32 pixels
constexpr int kPlanes = 4;                       // planes whose sums one thread keeps in registers
constexpr int kMaxGroups = 65535;                // gridDim.y: groups of kPlanes planes per launch; more take further launches
constexpr uint32_t kNaNBits = 0x7FC00000u;
static_assert(kTileW * kTileH == rg::kBlock, "one thread per pixel of the tile");

// ---- rain rate --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(rg::kBlock) void rain_rate_kernel(const float* __restrict__ src, const uint8_t* __restrict__ mask,
                                                               long n, double p, double q, double min_dbz, double max_dbz,
                                                               float* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = src[i];
  float r;
  if ((mask && mask[i]) || isnan(v)) {
    r = rg::bits_f32(kNaNBits);
  } else if (!((double)v >= min_dbz)) {
    r = 0.0f;
  } else {
    const double c = fmin((double)v, max_dbz);
    r = (float)exp(c * p - q);
  }
  out[i] = r;
}

// ---- accumulate -------------------------------------------------------------------------------------------------------------
// the samples of NP planes at one source position, as floats: what rg_advect_f32 writes there with a NaN fill
template <int METHOD, int NP>
__device__ __forceinline__ void sample_planes(const uint32_t* __restrict__ src, size_t plane, int h, int w, double fy, double fx,
                                              float (&v)[NP]) {
  if constexpr (METHOD == kBilinear) {
    const rg::BilinearTaps taps = rg::bilinear_taps(fx, fy, w, h, true);
#pragma unroll
    for (int p = 0; p < NP; ++p) v[p] = rg::bits_f32(rg::bilinear_sample(src + p * plane, w, taps, kNaNBits));
  } else {
    size_t at;
    const bool inside = rg::nearest_node(fx, fy, w, h, true, &at);
#pragma unroll
    for (int p = 0; p < NP; ++p) v[p] = rg::bits_f32(inside ? src[p * plane + at] : kNaNBits);
  }
}

// what depends on the sub-instant k alone, formed on the host in float64 exactly as the header writes it and passed by value:
// s = (k + 0.5) / n_steps, and the displacement's step for the two leads, s / substeps and (s - 1) / substeps.  Three float64
// divisions per sub-instant that every thread would otherwise repeat (float64 has no scalar unit to hoist them to).
struct Steps {
  double s[RG_MAX_ACC_STEPS], dt_prev[RG_MAX_ACC_STEPS], dt_next[RG_MAX_ACC_STEPS];
};

// one thread per pixel; blockIdx.x = the tile, row-major over tiles_x columns of tiles; blockIdx.y = a group of NP planes
// starting at plane0 + blockIdx.y * NP
template <int METHOD, int NP>
__global__ __launch_bounds__(rg::kBlock) void accumulate_kernel(const uint32_t* __restrict__ prev, const uint32_t* __restrict__ next,
                                                                int plane0, int h, int w, int tiles_x,
                                                                const float* __restrict__ motion,
                                                                rg_motion_lattice L, Steps steps, double hours, int n_steps, int substeps,
                                                                int min_steps, uint32_t fill, uint32_t* __restrict__ out,
                                                                uint8_t* __restrict__ out_steps) {
  const int tile_y = (int)(blockIdx.x / (unsigned)tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)tiles_x);
  const int x = tile_x * kTileW + (int)(threadIdx.x & (kTileW - 1));
  const int y = tile_y * kTileH + (int)(threadIdx.x / kTileW);
  if (x >= w || y >= h) return;
  const size_t plane = (size_t)h * w;
  const size_t first = ((size_t)plane0 + (size_t)blockIdx.y * NP) * plane;
  prev += first;
  next += first;
  const double py = (double)y, px = (double)x;
  double v0y, v0x;
  rg::motion_at(motion, L, py, px, &v0y, &v0x);

  double total[NP];
  int count[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    total[p] = 0.0;
    count[p] = 0;
  }
  for (int k = 0; k < n_steps; ++k) {
    const double s = steps.s[k];
    double dy, dx;
    float a[NP], b[NP];
    rg::displacement(motion, L, py, px, v0y, v0x, steps.dt_prev[k], substeps, &dy, &dx);
    sample_planes<METHOD, NP>(prev, plane, h, w, py - dy, px - dx, a);
    rg::displacement(motion, L, py, px, v0y, v0x, steps.dt_next[k], substeps, &dy, &dx);
    sample_planes<METHOD, NP>(next, plane, h, w, py - dy, px - dx, b);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const bool has_a = !isnan(a[p]), has_b = !isnan(b[p]);
      if (!(has_a || has_b)) continue;
      const double r = has_a && has_b ? (1.0 - s) * (double)a[p] + s * (double)b[p] : (double)(has_a ? a[p] : b[p]);
      total[p] += r;
      count[p] += 1;
    }
  }
  const size_t at = first + (size_t)y * w + x;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    out[at + p * plane] = count[p] >= min_steps ? rg::f32_bits((float)(hours * (total[p] / (double)count[p]))) : fill;
    if (out_steps) out_steps[at + p * plane] = (uint8_t)count[p];
  }
}

template <int METHOD, int NP>
void launch_accumulate(int groups, hipStream_t stream, const float* prev, const float* next, int plane0, int h, int w,
                       const float* motion, const rg_motion_lattice& L, const Steps& steps, double hours, int n_steps, int substeps,
                       int min_steps,
                       uint32_t fill, float* out, uint8_t* out_steps) {
  const int tiles_x = (w + kTileW - 1) / kTileW, tiles_y = (h + kTileH - 1) / kTileH;      // h * w < 2^31: the product fits
  const dim3 grid((unsigned)((int64_t)tiles_x * tiles_y), (unsigned)groups);
  hipLaunchKernelGGL((accumulate_kernel<METHOD, NP>), grid, dim3(rg::kBlock), 0, stream, reinterpret_cast<const uint32_t*>(prev),
                     reinterpret_cast<const uint32_t*>(next), plane0, h, w, tiles_x, motion, L, steps, hours, n_steps, substeps, min_steps, fill,
                     reinterpret_cast<uint32_t*>(out), out_steps);
}

// the remainder of n_planes % kPlanes planes, 1 .. kPlanes - 1 of them, behind the full groups
template <int METHOD, int NP = 1, class... A>
void launch_rest(int rest, A&&... args) {
  if constexpr (NP < kPlanes) {
    if (rest == NP)
      launch_accumulate<METHOD, NP>(1, args...);
    else
      launch_rest<METHOD, NP + 1>(rest, args...);
  }
}

int check_planes(const char* who, int32_t n, int32_t h, int32_t w, int64_t* total) {
  RG_REQUIRE(n >= 1, RG_EINVAL, "%s: the number of planes must be at least 1", who);
  RG_REQUIRE(h >= 0 && w >= 0, RG_EINVAL, "%s: negative size", who);
  *total = (int64_t)n * h * w;
  RG_REQUIRE(*total < (int64_t)1 << 31, RG_EINVAL, "%s: n * h * w must stay below 2^31", who);
  return RG_OK;
}

}  // namespace

extern "C" int rg_rain_rate_f32(const float* src, const uint8_t* mask, int32_t n, int32_t h, int32_t w, double p, double q,
                                double min_dbz, double max_dbz, float* out, rg_stream_t stream) {
  const char* who = "rg_rain_rate_f32";
  RG_REQUIRE(src && out, RG_EINVAL, "%s: null pointer", who);
  int64_t total;
  const int status = check_planes(who, n, h, w, &total);
  if (status != RG_OK) return status;
  RG_REQUIRE(isfinite(p) && p > 0.0, RG_EINVAL, "%s: p must be finite and positive", who);
  RG_REQUIRE(isfinite(q) && isfinite(min_dbz) && isfinite(max_dbz), RG_EINVAL, "%s: q, min_dbz and max_dbz must be finite", who);
  RG_REQUIRE(max_dbz >= min_dbz, RG_EINVAL, "%s: max_dbz lies below min_dbz", who);
  if (total == 0) return RG_OK;
  hipLaunchKernelGGL(rain_rate_kernel, dim3((unsigned)((total + rg::kBlock - 1) / rg::kBlock)), dim3(rg::kBlock), 0,
                     (hipStream_t)stream, src, mask, (long)total, p, q, min_dbz, max_dbz, out);
  return rg::check_launch(who);
}

extern "C" int rg_accumulate_advected_f32(const float* rate_prev, const float* rate_next, int32_t n_planes, int32_t h, int32_t w,
                                          const float* motion, rg_motion_lattice lattice, double hours, int32_t n_steps,
                                          int32_t substeps, int32_t method, int32_t min_steps, float fill, float* out,
                                          uint8_t* out_steps, rg_stream_t stream) {
  const char* who = "rg_accumulate_advected_f32";
  RG_REQUIRE(rate_prev && rate_next && motion && out, RG_EINVAL, "%s: null pointer", who);
  int64_t total;
  const int status = check_planes(who, n_planes, h, w, &total);
  if (status != RG_OK) return status;
  RG_REQUIRE(isfinite(lattice.origin_y) && isfinite(lattice.origin_x) && isfinite(lattice.step_y) && isfinite(lattice.step_x),
             RG_EINVAL, "%s: a member of rg_motion_lattice is not finite", who);
  RG_REQUIRE(lattice.step_y > 0.0 && lattice.step_x > 0.0, RG_EINVAL, "%s: step_y and step_x must be positive", who);
  RG_REQUIRE(lattice.ny >= 1 && lattice.nx >= 1, RG_EINVAL, "%s: ny and nx must be at least 1", who);
  RG_REQUIRE(isfinite(hours) && hours > 0.0, RG_EINVAL, "%s: hours must be finite and positive", who);
  RG_REQUIRE(n_steps >= 1 && n_steps <= RG_MAX_ACC_STEPS, RG_EINVAL, "%s: n_steps must lie in 1 .. %d", who, RG_MAX_ACC_STEPS);
  RG_REQUIRE(substeps >= 1 && substeps <= 16, RG_EINVAL, "%s: substeps must lie in 1 .. 16", who);
  RG_REQUIRE(method == kNearest || method == kBilinear, RG_EINVAL, "%s: unknown method %d", who, method);
  RG_REQUIRE(min_steps >= 1 && min_steps <= n_steps, RG_EINVAL, "%s: min_steps must lie in 1 .. n_steps", who);
  const int64_t field_bytes = (int64_t)lattice.ny * lattice.nx * 8;
  RG_REQUIRE(!rg::overlap(rate_prev, total * 4, out, total * 4) && !rg::overlap(rate_next, total * 4, out, total * 4) &&
                 !rg::overlap(motion, field_bytes, out, total * 4),
             RG_EINVAL, "%s: out overlaps an input", who);
  RG_REQUIRE(!out_steps || (!rg::overlap(rate_prev, total * 4, out_steps, total) && !rg::overlap(rate_next, total * 4, out_steps, total) &&
                            !rg::overlap(motion, field_bytes, out_steps, total)),
             RG_EINVAL, "%s: out_steps overlaps an input", who);
  RG_REQUIRE(!out_steps || !rg::overlap(out, total * 4, out_steps, total), RG_EINVAL, "%s: out_steps overlaps out", who);
  if (total == 0) return RG_OK;
  uint32_t fill_bits;
  memcpy(&fill_bits, &fill, sizeof fill_bits);
  Steps steps = {};
  for (int k = 0; k < n_steps; ++k) {
    steps.s[k] = ((double)k + 0.5) / (double)n_steps;
    steps.dt_prev[k] = steps.s[k] / (double)substeps;
    steps.dt_next[k] = (steps.s[k] - 1.0) / (double)substeps;
  }
  const int groups = n_planes / kPlanes, rest = n_planes % kPlanes;
  const hipStream_t s = (hipStream_t)stream;
  // the full groups in runs of at most kMaxGroups, each run one launch that starts at plane group0 * kPlanes; then the remainder
  for (int group0 = 0; group0 < groups; group0 += kMaxGroups) {
    const int run = groups - group0 < kMaxGroups ? groups - group0 : kMaxGroups;
    if (method == kNearest)
      launch_accumulate<kNearest, kPlanes>(run, s, rate_prev, rate_next, group0 * kPlanes, h, w, motion, lattice, steps, hours, n_steps,
                                           substeps, min_steps, fill_bits, out, out_steps);
    else
      launch_accumulate<kBilinear, kPlanes>(run, s, rate_prev, rate_next, group0 * kPlanes, h, w, motion, lattice, steps, hours, n_steps,
                                            substeps, min_steps, fill_bits, out, out_steps);
  }
  if (method == kNearest)
    launch_rest<kNearest>(rest, s, rate_prev, rate_next, groups * kPlanes, h, w, motion, lattice, steps, hours, n_steps, substeps, min_steps,
                          fill_bits, out, out_steps);
  else
    launch_rest<kBilinear>(rest, s, rate_prev, rate_next, groups * kPlanes, h, w, motion, lattice, steps, hours, n_steps, substeps,
                           min_steps, fill_bits, out, out_steps);
  return rg::check_launch(who);
}
