// Probabilistic nowcasts (include/radargrid_ensemble.h): the exceedance probabilities of an ensemble of extrapolations whose
// members differ by a shift per lead, and the counts a probability forecast is verified from.
//   exceedance   one thread per pixel and lead (blockIdx.y).  The displacement of rg_advect_f32 is formed once (the shared
//                rg_motion_field.hpp); each member then costs two float64 subtractions, one sample by the shared rules of
//                rg_sample.hpp and eight compares.  The shifts sit at wave-uniform addresses, so they arrive through the scalar
//                cache.  n_valid, the float64 sum and the eight counts -- eight 8-bit fields of one 64-bit register, since a count
//                reaches 64 -- never leave registers; every output plane of the pixel is written after the loop.  The M x L member
//                planes the per-member composition would store and read back do not exist.
//   histogram    the pattern of rg_contingency_f32 (rg_verify.hip): blockIdx.y = the plane, a bounded number of workgroups walks
//                it grid-stride, bins per workgroup in LDS, one 64-bit atomic per non-empty bin and workgroup.  Integer adds only,
//                so the result is exact in any order.
#include <math.h>

#include <algorithm>

#include "radargrid_ensemble.h"
#include "rg_common.hpp"
#include "rg_motion_field.hpp"
#include "rg_sample.hpp"

namespace {

#define RG_ENS_RELAXED __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

enum { kNearest = 0, kBilinear = 1 };

constexpr int kHistMaxStrips = 512;       // workgroups per plane of the histogram: the atomics one word receives
constexpr int kMaxBins = RG_MAX_VERIFY_THRESHOLDS * (RG_MAX_MEMBERS + 1) * 2;
constexpr uint32_t kNaNBits = 0x7FC00000u;

struct Leads {
  double v[RG_MAX_LEADS];
};

// thresholds by value: wave-uniform, read from scalar registers.  Entries from n on are NaN, which nothing exceeds.
struct Thresholds {
  float t[RG_MAX_VERIFY_THRESHOLDS];
};

// ---- exceedance --------------------------------------------------------------------------------------------------------------
template <int METHOD>
__global__ __launch_bounds__(rg::kBlock) void exceedance_kernel(const uint32_t* __restrict__ src, int h, int w,
                                                                const float* __restrict__ motion, rg_motion_lattice L, Leads leads,
                                                                int substeps, const double* __restrict__ shifts, int n_members,
                                                                Thresholds thr, int n_thr, int min_members,
                                                                float* __restrict__ prob, uint8_t* __restrict__ counts,
                                                                uint8_t* __restrict__ members, float* __restrict__ mean) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t plane = (size_t)h * w;
  if (i >= (long)plane) return;
  const int y = (int)(i / w), x = (int)(i - (long)y * w);
  const double py = (double)y, px = (double)x;
  double v0y, v0x, dy, dx;
  rg::motion_at(motion, L, py, px, &v0y, &v0x);
  rg::displacement(motion, L, py, px, v0y, v0x, leads.v[blockIdx.y] / (double)substeps, substeps, &dy, &dx);
  const double by = py - dy, bx = px - dx;                                  // the base position, once per pixel and lead
  const double* __restrict__ sh = shifts + (size_t)blockIdx.y * n_members * 2;      // wave-uniform
  unsigned long long packed = 0;                                            // cnt[t] in bits 8t .. 8t + 7
  int n_valid = 0;
  double sum = 0.0;
  for (int m = 0; m < n_members; ++m) {
    const double fy = by - sh[2 * m], fx = bx - sh[2 * m + 1];
    uint32_t bits;
    if constexpr (METHOD == kBilinear) {
      bits = rg::bilinear_sample(src, w, rg::bilinear_taps(fx, fy, w, h, true), kNaNBits);
    } else {
      size_t at;
      const bool inside = rg::nearest_node(fx, fy, w, h, true, &at);
      bits = inside ? src[at] : kNaNBits;
    }
    const float v = rg::bits_f32(bits);
    const bool present = !isnan(v);
    n_valid += present ? 1 : 0;
    sum = present ? sum + (double)v : sum;
#pragma unroll
    for (int t = 0; t < RG_MAX_VERIFY_THRESHOLDS; ++t) packed += (unsigned long long)(v >= thr.t[t] ? 1 : 0) << (8 * t);
  }
  const bool enough = n_valid >= min_members;
  const size_t lead_plane = (size_t)blockIdx.y * plane + (size_t)i;
  if (members) members[lead_plane] = (uint8_t)n_valid;
  if (mean) mean[lead_plane] = enough ? (float)(sum / (double)n_valid) : rg::bits_f32(kNaNBits);
#pragma unroll
  for (int t = 0; t < RG_MAX_VERIFY_THRESHOLDS; ++t) {
    if (t < n_thr) {
      const unsigned cnt = (unsigned)(packed >> (8 * t)) & 0xFFu;
      const size_t at = ((size_t)blockIdx.y * n_thr + t) * plane + (size_t)i;
      if (counts) counts[at] = (uint8_t)cnt;
      if (prob) prob[at] = enough ? (float)((double)cnt / (double)n_valid) : rg::bits_f32(kNaNBits);
    }
  }
}

// ---- histogram ---------------------------------------------------------------------------------------------------------------
// blockIdx.y = the plane, blockIdx.x = the strip; every wavefront walks whole groups of 64 pixels, so the ballot sees all lanes.
// bins[(t * (M + 1) + k) * 2 + o] is the layout of one plane of `hist`; bins[kMaxBins] counts the valid pixels.
__global__ __launch_bounds__(rg::kBlock) void histogram_kernel(const uint8_t* __restrict__ counts, const uint8_t* __restrict__ members,
                                                               const float* __restrict__ obs, const uint8_t* __restrict__ mask, int hw,
                                                               int M, Thresholds thr, int n_thr, long long* hist,
                                                               long long* valid_out) {
  __shared__ unsigned bins[kMaxBins + 1];
  const int lane = threadIdx.x % rg::kWave, wave = threadIdx.x / rg::kWave;
  const int n_bins = n_thr * (M + 1) * 2;
  for (int c = threadIdx.x; c <= kMaxBins; c += rg::kBlock) bins[c] = 0u;
  __syncthreads();
  const size_t plane = (size_t)blockIdx.y * (size_t)hw;
  unsigned n_ok = 0;
  const long step = (long)gridDim.x * rg::kBlock;
  for (long base = (long)blockIdx.x * rg::kBlock + wave * rg::kWave; base < hw; base += step) {
    const long i = base + lane;
    float o = 0.0f;
    bool ok = i < hw;
    if (ok) {
      o = obs[plane + i];
      ok = !isnan(o) && !(mask && mask[plane + i]) && (int)members[plane + i] == M;
    }
    unsigned k[RG_MAX_VERIFY_THRESHOLDS];
#pragma unroll
    for (int t = 0; t < RG_MAX_VERIFY_THRESHOLDS; ++t) {
      k[t] = 0u;
      if (t < n_thr && ok) k[t] = counts[(plane * n_thr + (size_t)t * hw) + i];
    }
#pragma unroll
    for (int t = 0; t < RG_MAX_VERIFY_THRESHOLDS; ++t) ok = ok && k[t] <= (unsigned)M;          // before any index is formed
    n_ok += (unsigned)__builtin_popcountll(__ballot(ok));
#pragma unroll
    for (int t = 0; t < RG_MAX_VERIFY_THRESHOLDS; ++t) {
      if (t < n_thr && ok) atomicAdd(&bins[(t * (M + 1) + (int)k[t]) * 2 + (o >= thr.t[t] ? 1 : 0)], 1u);
    }
  }
  if (lane == 0 && n_ok) atomicAdd(&bins[kMaxBins], n_ok);
  __syncthreads();
  for (int c = threadIdx.x; c < n_bins; c += rg::kBlock) {
    const unsigned total = bins[c];
    if (total) __hip_atomic_fetch_add(hist + (size_t)blockIdx.y * n_bins + c, (long long)total, RG_ENS_RELAXED);
  }
  if (threadIdx.x == 0 && bins[kMaxBins]) __hip_atomic_fetch_add(valid_out + blockIdx.y, (long long)bins[kMaxBins], RG_ENS_RELAXED);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
int read_thresholds(const char* who, const float* thresholds, int32_t n_thr, Thresholds* out) {
  RG_REQUIRE(n_thr >= 1 && n_thr <= RG_MAX_VERIFY_THRESHOLDS, RG_EINVAL, "%s: n_thr must lie in 1 .. %d, got %d", who,
             RG_MAX_VERIFY_THRESHOLDS, n_thr);
  for (int t = 0; t < RG_MAX_VERIFY_THRESHOLDS; ++t) {
    out->t[t] = t < n_thr ? thresholds[t] : NAN;
    RG_REQUIRE(t >= n_thr || isfinite(out->t[t]), RG_EINVAL, "%s: threshold %d is not finite", who, t);
  }
  return RG_OK;
}

int check_plane(const char* who, int32_t h, int32_t w) {
  RG_REQUIRE(h >= 0 && w >= 0, RG_EINVAL, "%s: negative size %d x %d", who, h, w);
  RG_REQUIRE((int64_t)h * w < ((int64_t)1 << 31), RG_EINVAL, "%s: h * w must stay below 2^31, got %d x %d", who, h, w);
  return RG_OK;
}

struct Span {
  const void* p;
  int64_t bytes;
  const char* name;
};

}  // namespace

extern "C" int rg_ensemble_exceedance_f32(const float* src, int32_t h, int32_t w, const float* motion, rg_motion_lattice lattice,
                                          const double* leads_host, int32_t n_leads, int32_t substeps, int32_t method,
                                          const double* shifts, int32_t n_members, const float* thresholds_host, int32_t n_thr,
                                          int32_t min_members, float* prob, uint8_t* counts, uint8_t* members, float* mean,
                                          rg_stream_t stream) {
  const char* who = "rg_ensemble_exceedance_f32";
  RG_REQUIRE(src && motion && thresholds_host && (leads_host || n_leads == 0) && (shifts || n_leads == 0), RG_EINVAL,
             "%s: null pointer", who);
  RG_REQUIRE(prob || counts || members || mean, RG_EINVAL, "%s: every output is NULL", who);
  int status = check_plane(who, h, w);
  if (status != RG_OK) return status;
  RG_REQUIRE(n_leads >= 0 && n_leads <= RG_MAX_LEADS, RG_EINVAL, "%s: n_leads must lie in 0 .. %d, got %d", who, RG_MAX_LEADS,
             n_leads);
  Leads leads = {};
  for (int l = 0; l < n_leads; ++l) {
    RG_REQUIRE(isfinite(leads_host[l]), RG_EINVAL, "%s: lead %d is not finite", who, l);
    leads.v[l] = leads_host[l];
  }
  RG_REQUIRE(isfinite(lattice.origin_y) && isfinite(lattice.origin_x) && isfinite(lattice.step_y) && isfinite(lattice.step_x),
             RG_EINVAL, "%s: a member of rg_motion_lattice is not finite", who);
  RG_REQUIRE(lattice.step_y > 0.0 && lattice.step_x > 0.0, RG_EINVAL, "%s: step_y and step_x must be positive", who);
  RG_REQUIRE(lattice.ny >= 1 && lattice.nx >= 1, RG_EINVAL, "%s: ny and nx must be at least 1", who);
  RG_REQUIRE(substeps >= 1 && substeps <= 16, RG_EINVAL, "%s: substeps must lie in 1 .. 16, got %d", who, substeps);
  RG_REQUIRE(method == kNearest || method == kBilinear, RG_EINVAL, "%s: unknown method %d", who, method);
  RG_REQUIRE(n_members >= 1 && n_members <= RG_MAX_MEMBERS, RG_EINVAL, "%s: n_members must lie in 1 .. %d, got %d", who,
             RG_MAX_MEMBERS, n_members);
  Thresholds thr;
  status = read_thresholds(who, thresholds_host, n_thr, &thr);
  if (status != RG_OK) return status;
  RG_REQUIRE(min_members >= 1 && min_members <= n_members, RG_EINVAL, "%s: min_members must lie in 1 .. n_members = %d, got %d", who,
             n_members, min_members);
  const int64_t hw = (int64_t)h * w, lead_planes = (int64_t)n_leads * hw, layers = lead_planes * n_thr;
  const Span in[] = {{src, hw * 4, "src"},
                     {motion, (int64_t)lattice.ny * lattice.nx * 8, "motion"},
                     {shifts, (int64_t)n_leads * n_members * 16, "shifts"}};
  const Span out[] = {{prob, layers * 4, "prob"}, {counts, layers, "counts"}, {members, lead_planes, "members"},
                      {mean, lead_planes * 4, "mean"}};
  for (int a = 0; a < 4; ++a) {
    if (!out[a].p) continue;
    for (const Span& s : in)
      RG_REQUIRE(!(s.p && rg::overlap(out[a].p, out[a].bytes, s.p, s.bytes)), RG_EINVAL, "%s: %s overlaps %s", who, out[a].name,
                 s.name);
    for (int b = a + 1; b < 4; ++b)
      RG_REQUIRE(!(out[b].p && rg::overlap(out[a].p, out[a].bytes, out[b].p, out[b].bytes)), RG_EINVAL, "%s: %s overlaps %s", who,
                 out[a].name, out[b].name);
  }
  if (hw == 0 || n_leads == 0) return RG_OK;
  const dim3 grid((unsigned)((hw + rg::kBlock - 1) / rg::kBlock), (unsigned)n_leads);
  const uint32_t* bits = reinterpret_cast<const uint32_t*>(src);
  if (method == kNearest)
    hipLaunchKernelGGL(exceedance_kernel<kNearest>, grid, dim3(rg::kBlock), 0, (hipStream_t)stream, bits, h, w, motion, lattice, leads,
                       substeps, shifts, n_members, thr, n_thr, min_members, prob, counts, members, mean);
  else
    hipLaunchKernelGGL(exceedance_kernel<kBilinear>, grid, dim3(rg::kBlock), 0, (hipStream_t)stream, bits, h, w, motion, lattice,
                       leads, substeps, shifts, n_members, thr, n_thr, min_members, prob, counts, members, mean);
  return rg::check_launch(who);
}

extern "C" int rg_ensemble_histogram_u8(const uint8_t* counts, const uint8_t* members, const float* obs, const uint8_t* mask,
                                        int32_t n_planes, int32_t h, int32_t w, int32_t n_members, const float* thresholds_host,
                                        int32_t n_thr, int64_t* hist, int64_t* valid, rg_stream_t stream) {
  const char* who = "rg_ensemble_histogram_u8";
  RG_REQUIRE(counts && members && obs && thresholds_host && hist && valid, RG_EINVAL, "%s: null pointer", who);
  RG_REQUIRE(n_planes >= 1 && n_planes <= 65535, RG_EINVAL, "%s: n_planes must lie in 1 .. 65535, got %d", who, n_planes);
  int status = check_plane(who, h, w);
  if (status != RG_OK) return status;
  RG_REQUIRE(n_members >= 1 && n_members <= RG_MAX_MEMBERS, RG_EINVAL, "%s: n_members must lie in 1 .. %d, got %d", who,
             RG_MAX_MEMBERS, n_members);
  Thresholds thr;
  status = read_thresholds(who, thresholds_host, n_thr, &thr);
  if (status != RG_OK) return status;
  const int64_t hw = (int64_t)h * w, planes = (int64_t)n_planes * hw;
  const int64_t hist_bytes = (int64_t)n_planes * n_thr * (n_members + 1) * 16, valid_bytes = (int64_t)n_planes * 8;
  RG_REQUIRE(!rg::overlap(hist, hist_bytes, valid, valid_bytes), RG_EINVAL, "%s: hist overlaps valid", who);
  const Span in[] = {{counts, planes * n_thr, "counts"}, {members, planes, "members"}, {obs, planes * 4, "obs"}, {mask, planes, "mask"}};
  for (const Span& s : in)
    RG_REQUIRE(!(s.p && (rg::overlap(hist, hist_bytes, s.p, s.bytes) || rg::overlap(valid, valid_bytes, s.p, s.bytes))), RG_EINVAL,
               "%s: an output overlaps %s", who, s.name);
  const hipStream_t s = (hipStream_t)stream;
  rg::fill_words(hist, hist_bytes, 0u, s);
  rg::fill_words(valid, valid_bytes, 0u, s);
  if (hw == 0) return rg::check_launch(who);
  const unsigned strips = (unsigned)std::min<int64_t>((hw + rg::kBlock - 1) / rg::kBlock, kHistMaxStrips);
  hipLaunchKernelGGL(histogram_kernel, dim3(strips, (unsigned)n_planes), dim3(rg::kBlock), 0, s, counts, members, obs, mask, (int)hw,
                     n_members, thr, n_thr, reinterpret_cast<long long*>(hist), reinterpret_cast<long long*>(valid));
  return rg::check_launch(who);
}
