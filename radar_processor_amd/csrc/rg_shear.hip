// Azimuthal shear and radial divergence by local linear least squares, and the median pre-filter (include/radargrid_shear.h).
//
// The median is pointwise over a window of at most 5 x 5: one thread per gate, the window in registers, sorted by a fixed
// network of compare-exchanges (odd-even transposition; invalid gates are +inf pads that end up last).
//
// The LLSD is the kernel with a hot path.  A workgroup takes kTileG gates of kBandR consecutive rays plus a halo of H rays on
// either side, H the largest clamped half_rays[] among the tile's own gates.  The nine window sums separate: for a ray a' and a
// centre gate g the range-window sums (n, Sj, Sjj, Sq, Sjq) do not depend on the centre ray, and the nine sums of a window are
// those five combined over 2 * ka + 1 rays with weights 1, i, i * i.
//   load     every ray of the tile and its halo x (kTileG + 2 * half_gates) gates -> registers, all loads in flight at once
//   stage    the fixed-point values of kChunk rays at a time -> LDS (kInvalid where not valid)
//   range    a thread takes kSeg consecutive gates of one staged ray: the first window is summed, the next ones slide
//            (remove the gate that leaves, shift every offset by one, add the gate that enters); entries -> LDS
//   fit      a thread per gate of the tile: its column of 2 * ka + 1 entries, the nine sums, the fit in float64
// LDS images (banking: cdna_hip_programming.md section 2).  The stage has rows of 65 words: the 32 lanes of a half-wave hold 32
// different rows at one column, 65 = 1 (mod 32), so ds_read_b32 is conflict-free.  The entries are three arrays of 8-byte
// words with rows of 33 words: a range thread's 16-lane group writes 16 different rows at one gate, 66 dwords apart -- 16
// different even banks; the fit reads 32 consecutive gates of one row per half-wave -- the 64 banks once.
// Every sum is an integer, so no order of summation matters (bounds: the header).
#include <math.h>

#include "radargrid_shear.h"
#include "rg_common.hpp"

namespace {

constexpr uint32_t kQuietNaN = 0x7FC00000u;
constexpr int kInvalid = INT32_MIN;                           // |q| <= 2^30: never a fixed-point value

constexpr int kTileG = 32;                                    // gates of a tile
constexpr int kBandR = 40;                                    // rays of a tile
constexpr int kRows = kBandR + 2 * RG_SHEAR_MAX_HALF_RAYS;    // 72: rays of a tile and its largest halo
constexpr int kStride = kTileG + 1;                           // 8-byte words per row of entries
constexpr int kChunk = 32;                                    // rays staged at a time
constexpr int kStageW = kTileG + 2 * RG_SHEAR_MAX_HALF_GATES; // 64: gates of a staged ray at most
constexpr int kStageStride = kStageW + 1;
constexpr int kSeg = 4;                                       // consecutive gates one range thread slides over
static_assert(kChunk * (kTileG / kSeg) == rg::kBlock, "one range thread per (staged ray, segment)");
static_assert(kStageW == rg::kWave, "a wavefront stages one ray per step");
constexpr int kWaves = rg::kBlock / rg::kWave;                // 4
constexpr int kLoads = (kRows + kWaves - 1) / kWaves;         // 18: rays one wavefront loads
static_assert(kChunk % kWaves == 0, "a chunk is whole steps of the wavefronts");

struct alignas(8) Geo {                                       // the integer sums of one ray's range window
  short n, sj;                                                // n <= 33, |Sj| <= 136
  int sjj;                                                    // <= 2992
};

// finite and |v| <= RG_VELOCITY_MAX_ABS: both fail for NaN, the second for +-inf
__device__ __forceinline__ bool valid_value(float v) { return fabsf(v) <= (float)RG_VELOCITY_MAX_ABS; }

__device__ __forceinline__ float quiet(float v) { return v != v ? rg::bits_f32(kQuietNaN) : v; }

// ---- 1  median -------------------------------------------------------------------------------------------------------------------
template <int HR, int HG>
__global__ __launch_bounds__(rg::kBlock) void median_kernel(const float* __restrict__ vel, const uint8_t* __restrict__ mask, int R,
                                                            int G, long n_gates, int wrap_rays, int min_valid, int centre_only,
                                                            float* __restrict__ out) {
  constexpr int N = (2 * HR + 1) * (2 * HG + 1);
  const long at = (long)blockIdx.x * rg::kBlock + threadIdx.x;
  if (at >= n_gates) return;
  const int g = (int)(at % G);
  const long ray = at / G;
  const int a = (int)(ray % R);
  const long sweep = (ray - a) * G;                           // flat index of the sweep's first gate
  const float kPad = __builtin_inff();                         // sorts behind every valid value
  float w[N];
  bool centre_valid = false;
  int n = 0;
#pragma unroll
  for (int i = -HR; i <= HR; ++i) {
    int ai = a + i;
    bool in_ray = true;
    if (wrap_rays) {
      ai = ai < 0 ? ai + R : ai >= R ? ai - R : ai;           // 2 * HR + 1 <= R: one turn at most
    } else {
      in_ray = ai >= 0 && ai < R;
    }
#pragma unroll
    for (int j = -HG; j <= HG; ++j) {
      const int k = (i + HR) * (2 * HG + 1) + (j + HG);
      const int gj = g + j;
      float v = kPad;
      bool ok = in_ray && gj >= 0 && gj < G;
      if (ok) {
        const long idx = sweep + (long)ai * G + gj;
        v = vel[idx];
        ok = valid_value(v) && !(mask && mask[idx]);
      }
      w[k] = ok ? v : kPad;
      if (ok) ++n;
      if (i == 0 && j == 0) centre_valid = ok;
    }
  }
  float result = rg::bits_f32(kQuietNaN);
  if (n >= min_valid && (!centre_only || centre_valid)) {
    // odd-even transposition: N rounds of compare-exchange by compare and select (the bits of an input are never changed); the
    // pads end up behind the n valid values
#pragma unroll
    for (int round = 0; round < N; ++round) {
#pragma unroll
      for (int k = round & 1; k + 1 < N; k += 2) {
        const float lo = w[k], hi = w[k + 1];
        const bool swap = hi < lo;
        w[k] = swap ? hi : lo;
        w[k + 1] = swap ? lo : hi;
      }
    }
    const int target = (n - 1) / 2;
#pragma unroll
    for (int k = 0; k < (N + 1) / 2; ++k)
      if (k == target) result = w[k];
  }
  out[at] = result;
}

// ---- 2  LLSD ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(rg::kBlock) void llsd_kernel(const float* __restrict__ vel, const uint8_t* __restrict__ mask, int R,
                                                          int G, unsigned tiles_g, unsigned bands,
                                                          const int* __restrict__ half_rays, const double* __restrict__ az_scale,
                                                          int max_half_rays, int hg, double range_scale, int wrap_rays,
                                                          int min_valid, int min_fraction_q16, int centre_only,
                                                          float* __restrict__ az_shear, float* __restrict__ divergence,
                                                          float* __restrict__ vel_s, uint16_t* __restrict__ count) {
  __shared__ Geo s_geo[kRows * kStride];
  __shared__ long long s_sq[kRows * kStride];
  __shared__ long long s_sjq[kRows * kStride];
  __shared__ int s_stage[kChunk * kStageStride];
  __shared__ int s_halo;

  const int tid = threadIdx.x;
  // the tile of gates is the SLOWEST index: the nearest tiles, whose windows and halos are the widest, start first
  unsigned b = blockIdx.x;
  const int a0 = (int)(b % bands) * kBandR;
  b /= bands;
  const unsigned n_sweeps = gridDim.x / (tiles_g * bands);
  const long sweep = (long)(b % n_sweeps) * R * G;            // flat index of the sweep's first gate
  const int g0 = (int)(b / n_sweeps) * kTileG;
  const int rays_here = R - a0 < kBandR ? R - a0 : kBandR;

  // the halo: the largest clamped half-width among the tile's own gates
  if (tid == 0) s_halo = 0;
  __syncthreads();
  if (tid < kTileG && g0 + tid < G) {
    int ka = half_rays[g0 + tid];
    ka = ka < 0 ? 0 : ka > max_half_rays ? max_half_rays : ka;
    atomicMax(&s_halo, ka);
  }
  __syncthreads();
  const int halo = s_halo;
  const int rows = rays_here + 2 * halo;                      // <= kRows; local row lr is ray a0 - halo + lr
  const int width = kTileG + 2 * hg;                          // staged gates: g0 - hg .. g0 + kTileG + hg - 1

  // load: a wavefront per ray, a lane per gate; every load of the workgroup is issued before the first value is used, so the
  // tile and its halo cost one trip to memory, not one per staged ray
  const int col = tid % rg::kWave, wave = tid / rg::kWave;
  float v[kLoads];
  uint8_t m[kLoads];
#pragma unroll
  for (int t = 0; t < kLoads; ++t) {
    const int lr = wave + kWaves * t;
    int a = a0 - halo + lr;
    const int g = g0 - hg + col;
    bool in = lr < rows && col < width && g >= 0 && g < G;
    if (wrap_rays) {
      a = a < 0 ? a + R : a >= R ? a - R : a;                 // -halo <= a < R + halo and 2 * halo + 1 <= R: one turn at most
    } else {
      in = in && a >= 0 && a < R;
    }
    v[t] = __builtin_nanf("");
    m[t] = 0;
    if (in) {
      const long idx = sweep + (long)a * G + g;
      v[t] = vel[idx];
      if (mask) m[t] = mask[idx];
    }
  }
  int q[kLoads];
#pragma unroll
  for (int t = 0; t < kLoads; ++t) q[t] = valid_value(v[t]) && !m[t] ? (int)llrint(65536.0 * (double)v[t]) : kInvalid;

#pragma unroll
  for (int c = 0; c < (kRows + kChunk - 1) / kChunk; ++c) {
    const int c0 = c * kChunk;
    if (c0 >= rows) break;
    // stage the chunk's rays
#pragma unroll
    for (int it = 0; it < kChunk / kWaves; ++it) {
      const int t = c * (kChunk / kWaves) + it;
      if (t < kLoads) {
        const int row = wave + kWaves * it;
        if (c0 + row < rows && col < width) s_stage[row * kStageStride + col] = q[t];
      }
    }
    __syncthreads();
    // range: the windows of kSeg consecutive gates of one staged ray.  The window of local gate c holds stage columns c .. c + 2 hg
    {
      const int row = tid % kChunk, c_first = (tid / kChunk) * kSeg;
      const int lr = c0 + row;
      if (lr < rows) {
        const int* stage = s_stage + row * kStageStride;
        int n = 0, sj = 0, sjj = 0;
        long long sq = 0, sjq = 0;
        for (int j = -hg; j <= hg; ++j) {
          const int q = stage[c_first + hg + j];
          if (q != kInvalid) {
            n += 1;
            sj += j;
            sjj += j * j;
            sq += q;
            sjq += (long long)j * q;
          }
        }
        for (int m = 0;; ++m) {
          const int at = lr * kStride + c_first + m;
          Geo e;
          e.n = (short)n;
          e.sj = (short)sj;
          e.sjj = sjj;
          s_geo[at] = e;
          s_sq[at] = sq;
          s_sjq[at] = sjq;
          if (m == kSeg - 1) break;
          const int leaves = stage[c_first + m], enters = stage[c_first + m + 1 + 2 * hg];
          if (leaves != kInvalid) {                           // offset -hg
            n -= 1;
            sj += hg;
            sjj -= hg * hg;
            sq -= leaves;
            sjq += (long long)hg * leaves;
          }
          sjj += n - 2 * sj;                                  // every offset j becomes j - 1
          sj -= n;
          sjq -= sq;
          if (enters != kInvalid) {                           // offset +hg
            n += 1;
            sj += hg;
            sjj += hg * hg;
            sq += enters;
            sjq += (long long)hg * enters;
          }
        }
      }
    }
    __syncthreads();
  }

  // fit: a lane per gate of the tile, kBlock / kTileG rays per step
  const int gl = tid % kTileG;
  const int g = g0 + gl;
  if (g >= G) return;
  int ka = half_rays[g];
  ka = ka < 0 ? 0 : ka > max_half_rays ? max_half_rays : ka;
  const double scale = az_scale[g];
  const long long window = (long long)(2 * ka + 1) * (2 * hg + 1);
  for (int ar = tid / kTileG; ar < rays_here; ar += rg::kBlock / kTileG) {
    const int lr = halo + ar;
    int n = 0, si = 0, sj = 0, sii = 0, sij = 0, sjj = 0;
    long long sq = 0, siq = 0, sjq = 0;
    for (int i = -ka; i <= ka; ++i) {
      const int at = (lr + i) * kStride + gl;
      const Geo e = s_geo[at];
      const long long q1 = s_sq[at], q2 = s_sjq[at];
      n += e.n;
      si += i * e.n;
      sj += e.sj;
      sii += i * i * e.n;
      sij += i * e.sj;
      sjj += e.sjj;
      sq += q1;
      siq += i * q1;
      sjq += q2;
    }
    const long idx = sweep + (long)(a0 + ar) * G + g;
    bool defined = n >= min_valid && (long long)n * 65536 >= (long long)min_fraction_q16 * window;
    if (defined && centre_only) defined = valid_value(vel[idx]) && !(mask && mask[idx]);
    const long long A = (long long)n * sii - (long long)si * si, B = (long long)n * sij - (long long)si * sj,
                    C = (long long)n * sjj - (long long)sj * sj;
    const long long D = A * C - B * B;
    defined = defined && D > 0;
    float shear = rg::bits_f32(kQuietNaN), div = shear, smooth = shear;
    if (defined) {
      const long long P = n * siq - si * sq, Q = n * sjq - sj * sq;
      const double al = ((double)P * (double)C - (double)Q * (double)B) / (double)D;
      const double be = ((double)Q * (double)A - (double)P * (double)B) / (double)D;
      shear = quiet((float)(al * scale));
      div = quiet((float)(be * range_scale));
      if (vel_s) smooth = quiet((float)(((((double)sq - al * (double)si) - be * (double)sj) / (double)n) / 65536.0));
    }
    if (az_shear) az_shear[idx] = shear;
    if (divergence) divergence[idx] = div;
    if (vel_s) vel_s[idx] = smooth;
    if (count) count[idx] = (uint16_t)n;
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
struct Span {
  const void* p;
  int64_t bytes;
  const char* name;
};

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// S, R >= 1, G >= 0 and S * R * G < 2^31
int check_volume(const char* who, int32_t S, int32_t R, int32_t G) {
  RG_REQUIRE(S >= 1 && R >= 1, RG_EINVAL, "%s: S and R must be at least 1, got %d and %d", who, S, R);
  RG_REQUIRE(G >= 0, RG_EINVAL, "%s: G must not be negative, got %d", who, G);
  RG_REQUIRE((__int128)S * R * G < ((__int128)1 << 31), RG_EINVAL, "%s: %d sweeps of %d x %d are 2^31 gates or more", who, S, R, G);
  return RG_OK;
}

// no output overlaps an input or another output
int check_overlaps(const char* who, const Span* in, int n_in, const Span* out, int n_out) {
  for (int a = 0; a < n_out; ++a) {
    if (!out[a].p) continue;
    for (int b = 0; b < n_in; ++b)
      RG_REQUIRE(!(in[b].p && rg::overlap(out[a].p, out[a].bytes, in[b].p, in[b].bytes)), RG_EINVAL, "%s: %s overlaps %s", who,
                 out[a].name, in[b].name);
    for (int b = a + 1; b < n_out; ++b)
      RG_REQUIRE(!(out[b].p && rg::overlap(out[a].p, out[a].bytes, out[b].p, out[b].bytes)), RG_EINVAL, "%s: %s overlaps %s", who,
                 out[a].name, out[b].name);
  }
  return RG_OK;
}

template <int HR, int HG>
void launch_median(const float* vel, const uint8_t* mask, int R, int G, long n, int wrap_rays, int min_valid, int centre_only,
                   float* out, hipStream_t s) {
  hipLaunchKernelGGL((median_kernel<HR, HG>), dim3((unsigned)((n + rg::kBlock - 1) / rg::kBlock)), dim3(rg::kBlock), 0, s, vel, mask,
                     R, G, n, wrap_rays, min_valid, centre_only, out);
}

}  // namespace

extern "C" int rg_polar_median_f32(const float* vel, const uint8_t* mask, int32_t S, int32_t R, int32_t G, int32_t half_rays,
                                   int32_t half_gates, int32_t wrap_rays, int32_t min_valid, int32_t centre_only, float* out,
                                   rg_stream_t stream) {
  const char* who = "rg_polar_median_f32";
  RG_REQUIRE(vel && out, RG_EINVAL, "%s: null pointer", who);
  int status = check_volume(who, S, R, G);
  if (status != RG_OK) return status;
  RG_REQUIRE(half_rays >= 0 && half_rays <= RG_SHEAR_MEDIAN_MAX_HALF && half_gates >= 0 && half_gates <= RG_SHEAR_MEDIAN_MAX_HALF,
             RG_EINVAL, "%s: half_rays and half_gates must lie in 0 .. %d, got %d and %d", who, RG_SHEAR_MEDIAN_MAX_HALF, half_rays,
             half_gates);
  RG_REQUIRE(half_rays > 0 || half_gates > 0, RG_EINVAL, "%s: half_rays and half_gates are both 0", who);
  RG_REQUIRE(!wrap_rays || 2 * half_rays + 1 <= R, RG_EINVAL, "%s: a window of %d rays does not fit a circle of %d rays", who,
             2 * half_rays + 1, R);
  RG_REQUIRE(min_valid >= 1 && min_valid <= 25, RG_EINVAL, "%s: min_valid must lie in 1 .. 25, got %d", who, min_valid);
  const int64_t n = (int64_t)S * R * G;
  const Span in[] = {{vel, n * 4, "vel"}, {mask, n, "mask"}};
  const Span outs[] = {{out, n * 4, "out"}};
  status = check_overlaps(who, in, 2, outs, 1);
  if (status != RG_OK) return status;
  if (G == 0) return RG_OK;
  hipStream_t s = (hipStream_t)stream;
  const int wrap = wrap_rays ? 1 : 0, centre = centre_only ? 1 : 0;
#define RG_MEDIAN_CASE(HR, HG) \
  case (HR) * 3 + (HG):        \
    launch_median<HR, HG>(vel, mask, R, G, (long)n, wrap, min_valid, centre, out, s); \
    break
  switch (half_rays * 3 + half_gates) {
    RG_MEDIAN_CASE(0, 1);
    RG_MEDIAN_CASE(0, 2);
    RG_MEDIAN_CASE(1, 0);
    RG_MEDIAN_CASE(1, 1);
    RG_MEDIAN_CASE(1, 2);
    RG_MEDIAN_CASE(2, 0);
    RG_MEDIAN_CASE(2, 1);
    RG_MEDIAN_CASE(2, 2);
  }
#undef RG_MEDIAN_CASE
  return rg::check_launch(who);
}

extern "C" int rg_velocity_llsd_f32(const float* vel, const uint8_t* mask, int32_t S, int32_t R, int32_t G, const int32_t* half_rays,
                                    const double* az_scale, int32_t max_half_rays, int32_t half_gates, double range_scale,
                                    int32_t wrap_rays, int32_t min_valid, int32_t min_fraction_q16, int32_t centre_only,
                                    float* az_shear, float* divergence, float* vel_s, uint16_t* count, rg_stream_t stream) {
  const char* who = "rg_velocity_llsd_f32";
  RG_REQUIRE(vel && half_rays && az_scale, RG_EINVAL, "%s: null pointer", who);
  RG_REQUIRE(az_shear || divergence || vel_s, RG_EINVAL, "%s: none of az_shear, divergence and vel_s is asked for", who);
  int status = check_volume(who, S, R, G);
  if (status != RG_OK) return status;
  RG_REQUIRE(max_half_rays >= 1 && max_half_rays <= RG_SHEAR_MAX_HALF_RAYS, RG_EINVAL, "%s: max_half_rays must lie in 1 .. %d, got %d",
             who, RG_SHEAR_MAX_HALF_RAYS, max_half_rays);
  RG_REQUIRE(half_gates >= 1 && half_gates <= RG_SHEAR_MAX_HALF_GATES, RG_EINVAL, "%s: half_gates must lie in 1 .. %d, got %d", who,
             RG_SHEAR_MAX_HALF_GATES, half_gates);
  RG_REQUIRE(!wrap_rays || 2 * max_half_rays + 1 <= R, RG_EINVAL, "%s: a window of %d rays does not fit a circle of %d rays", who,
             2 * max_half_rays + 1, R);
  RG_REQUIRE(min_valid >= 3 && min_valid <= RG_SHEAR_MAX_WINDOW, RG_EINVAL, "%s: min_valid must lie in 3 .. %d, got %d", who,
             RG_SHEAR_MAX_WINDOW, min_valid);
  RG_REQUIRE(min_fraction_q16 >= 0 && min_fraction_q16 <= 65536, RG_EINVAL, "%s: min_fraction_q16 must lie in 0 .. 65536, got %d", who,
             min_fraction_q16);
  RG_REQUIRE(isfinite(range_scale), RG_EINVAL, "%s: range_scale must be finite, got %g", who, range_scale);
  RG_REQUIRE(aligned_to(az_scale, 8), RG_EALIGN, "%s: az_scale must be 8-byte aligned", who);
  const int64_t n = (int64_t)S * R * G;
  const Span in[] = {{vel, n * 4, "vel"}, {mask, n, "mask"}, {half_rays, (int64_t)G * 4, "half_rays"}, {az_scale, (int64_t)G * 8, "az_scale"}};
  const Span outs[] = {{az_shear, n * 4, "az_shear"}, {divergence, n * 4, "divergence"}, {vel_s, n * 4, "vel_s"}, {count, n * 2, "count"}};
  status = check_overlaps(who, in, 4, outs, 4);
  if (status != RG_OK) return status;
  if (G == 0) return RG_OK;
  const unsigned tiles_g = (unsigned)((G + kTileG - 1) / kTileG), bands = (unsigned)((R + kBandR - 1) / kBandR);
  const int64_t blocks = (int64_t)tiles_g * bands * S;        // every workgroup holds a gate: fewer than 2^31
  hipLaunchKernelGGL(llsd_kernel, dim3((unsigned)blocks), dim3(rg::kBlock), 0, (hipStream_t)stream, vel, mask, R, G, tiles_g, bands,
                     half_rays, az_scale, max_half_rays, half_gates, range_scale, wrap_rays ? 1 : 0, min_valid, min_fraction_q16,
                     centre_only ? 1 : 0, az_shear, divergence, vel_s, count);
  return rg::check_launch(who);
}
