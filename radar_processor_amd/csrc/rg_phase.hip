// Differential phase in the polar domain (include/radargrid_phase.h): unfold PHIDP, fit it with a windowed least-squares line
// (smoothed PHIDP and KDP), correct Z and ZDR for path-integrated attenuation.  All three are scans along a ray.
//   unfold        one wavefront per ray, trips of 64 gates (the shape of echo_rows_kernel, rg_convection.hip).  The previous
//                 valid value is a ballot plus one shuffle from the nearest lower set lane; the fold count K is a shuffle
//                 ladder; the last valid value and K are carried across trips in scalar registers.
//   fit           no table in HBM.  A workgroup takes kFitTile gates of one ray plus a halo of 255 on either side, builds
//                 tile-relative prefixes of (valid, t, t^2, q, t * q) in LDS -- each wavefront scans a quarter of the span with
//                 the ladder, the quarters' totals are added before the one write -- and every lane takes two prefix reads per
//                 sum.  The sums are re-centred on the lane's own gate (j = t - c): integers, so exact.
//   attenuation   one wavefront per ray again: "first defined" is a ballot and a shuffle, the running maximum a ladder.
// Every sum is an integer and max is exact in any order: the outputs are bit-reproducible.
#include <math.h>

#include "radargrid_phase.h"
#include "rg_common.hpp"

namespace {

constexpr int kWavesPerBlock = rg::kBlock / rg::kWave;      // rays of a workgroup in the two row-scan kernels
constexpr uint32_t kNaNBits = 0x7FC00000u;

constexpr int kHalo = RG_PHASE_MAX_HALF_WINDOW;
constexpr int kFitTile = 2 * rg::kBlock;                    // gates of a ray one workgroup fits: two per thread
constexpr int kFitSpan = kFitTile + 2 * kHalo;              // 1022 gates are scanned for them
constexpr int kFitTrips = 4;                                // trips of 64 per wavefront: 4 waves x 4 x 64 = 1024 >= kFitSpan
static_assert(kWavesPerBlock * kFitTrips * rg::kWave >= kFitSpan, "the four wavefronts cover the span");
// the header's overflow rule: with N <= 2L + 1, |j| <= L and |q| <= 2^30, N * Sjq and Sj * Sq stay below 2^57
constexpr long long kMaxN = 2 * kHalo + 1, kMaxSj = (long long)kHalo * (kHalo + 1), kMaxQ = 1ll << 30;
static_assert((long long)RG_PHASE_MAX_ABS_PHI * 65536 == kMaxQ, "q = 65536 * phi fits 2^30");
static_assert(kMaxN * (kMaxSj * kMaxQ) < (1ll << 57) && kMaxSj * (kMaxN * kMaxQ) < (1ll << 57), "num fits int64");
// the tile-relative prefixes: t < 1024, so sum t * q < 2^10 * 2^10 * 2^30 and sum t^2 < 2^31
static_assert((long long)kFitSpan * kFitSpan * kMaxQ < (1ll << 51) && (long long)kFitSpan * kFitSpan * kFitSpan / 3 < (1ll << 31),
              "the LDS prefixes fit their types");

// n_classes - 1 edges already rounded to float32; the rest are +inf, which no dbz reaches.  By value: wave-uniform.
struct Windows {
  float edge[RG_PHASE_MAX_CLASSES - 1];
  int half[RG_PHASE_MAX_CLASSES];
};

__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

// ---- unfold ------------------------------------------------------------------------------------------------------------------
// phidp and out may be the same array: a lane reads its gate before it writes it and never reads another lane's gate from memory.
__global__ __launch_bounds__(rg::kBlock) void unfold_kernel(const float* phidp, const uint8_t* __restrict__ mask, int R, int G,
                                                            double wrap, float half, float* out, int* __restrict__ folds) {
  const int lane = threadIdx.x % rg::kWave;
  const long row = (long)blockIdx.x * kWavesPerBlock + threadIdx.x / rg::kWave;
  if (row >= R) return;                                                               // the whole wavefront
  const size_t in_row = (size_t)row * (size_t)G;
  const unsigned long long below = lanes_below(lane);
  float carry_v = 0.0f;            // the last valid value of the trips before
  bool carry_has = false;
  int carry_K = 0;
  for (int x0 = 0; x0 < G; x0 += rg::kWave) {
    const int x = x0 + lane;
    const bool in = x < G;
    float v = 0.0f;
    bool valid = false;
    if (in) {
      v = phidp[in_row + x];
      valid = isfinite(v) && !(mask && mask[in_row + x]);
    }
    const unsigned long long hit = __ballot(valid);
    const unsigned long long lower = hit & below;
    const int from = lower ? 63 - __builtin_clzll(lower) : 0;
    const float near = __shfl(v, from);                                               // every lane takes part
    const bool has = lower != 0 || carry_has;
    const float prev = lower ? near : carry_v;
    int k = 0;
    if (valid && has) {
      const float d = v - prev;
      k = d > half ? -1 : (d < -half ? 1 : 0);
    }
#pragma unroll
    for (int s = 1; s < rg::kWave; s <<= 1) {
      const int t = __shfl_up(k, s);
      if (lane >= s) k += t;
    }
    const int K = carry_K + k;
    if (in) {
      out[in_row + x] = valid ? (float)((double)v + (double)K * wrap) : rg::bits_f32(kNaNBits);
      if (folds) folds[in_row + x] = valid ? K : 0;
    }
    carry_K += __shfl(k, rg::kWave - 1);
    if (hit) {                                                                        // wave-uniform
      carry_v = __shfl(v, 63 - __builtin_clzll(hit));
      carry_has = true;
    }
  }
}

// ---- fit ---------------------------------------------------------------------------------------------------------------------
// blockIdx.x = ray * tiles + tile.  Entry e of the span is gate tile * kFitTile - kHalo + e; prefix index e + 1 holds the sums
// over the entries 0 .. e, index 0 holds zeros.  Gates outside the ray are invalid entries.
__global__ __launch_bounds__(rg::kBlock) void fit_kernel(const float* __restrict__ phi, int G, int tiles,
                                                         const float* __restrict__ dbz, Windows win, int min_valid, int centre_only,
                                                         double scale, float* __restrict__ kdp, float* __restrict__ phi_s,
                                                         uint16_t* __restrict__ count) {
  __shared__ long long p_q[kFitSpan + 3], p_tq[kFitSpan + 3];
  __shared__ int p_n[kFitSpan + 3], p_t[kFitSpan + 3], p_tt[kFitSpan + 3];
  __shared__ long long tot_q[kWavesPerBlock], tot_tq[kWavesPerBlock];
  __shared__ int tot_n[kWavesPerBlock], tot_t[kWavesPerBlock], tot_tt[kWavesPerBlock];
  const int lane = threadIdx.x % rg::kWave, wave = threadIdx.x / rg::kWave;
  const unsigned ray = blockIdx.x / (unsigned)tiles, tile = blockIdx.x - ray * (unsigned)tiles;
  const size_t in_row = (size_t)ray * (size_t)G;
  const int g0 = (int)tile * kFitTile - kHalo;                        // the gate of entry 0
  const unsigned long long upto = lanes_below(lane) | (1ull << lane);

  // each wavefront scans its quarter of the span; the inclusive prefixes of its four trips stay in registers
  long long q_[kFitTrips], tq_[kFitTrips];
  int n_[kFitTrips], t_[kFitTrips], tt_[kFitTrips];
  long long cq = 0, ctq = 0;
  int cn = 0, ct = 0, ctt = 0;
#pragma unroll
  for (int trip = 0; trip < kFitTrips; ++trip) {
    const int e = (wave * kFitTrips + trip) * rg::kWave + lane, g = g0 + e;
    long long q = 0;
    bool valid = false;
    if (e < kFitSpan && g >= 0 && g < G) {
      const float v = phi[in_row + g];
      valid = isfinite(v) && fabsf(v) <= (float)RG_PHASE_MAX_ABS_PHI;
      if (valid) q = llrint(65536.0 * (double)v);
    }
    const unsigned long long hit = __ballot(valid);
    long long tq = (long long)e * q;
    int t = valid ? e : 0, tt = valid ? e * e : 0;
#pragma unroll
    for (int s = 1; s < rg::kWave; s <<= 1) {
      const long long aq = __shfl_up(q, s), atq = __shfl_up(tq, s);
      const int at = __shfl_up(t, s), att = __shfl_up(tt, s);
      if (lane >= s) {
        q += aq;
        tq += atq;
        t += at;
        tt += att;
      }
    }
    q_[trip] = cq + q;
    tq_[trip] = ctq + tq;
    n_[trip] = cn + __builtin_popcountll(hit & upto);
    t_[trip] = ct + t;
    tt_[trip] = ctt + tt;
    cq += __shfl(q, rg::kWave - 1);
    ctq += __shfl(tq, rg::kWave - 1);
    cn += __builtin_popcountll(hit);
    ct += __shfl(t, rg::kWave - 1);
    ctt += __shfl(tt, rg::kWave - 1);
  }
  if (lane == 0) {
    tot_q[wave] = cq;
    tot_tq[wave] = ctq;
    tot_n[wave] = cn;
    tot_t[wave] = ct;
    tot_tt[wave] = ctt;
  }
  __syncthreads();
  long long bq = 0, btq = 0;                                          // the quarters before this one
  int bn = 0, bt = 0, btt = 0;
  for (int w = 0; w < wave; ++w) {
    bq += tot_q[w];
    btq += tot_tq[w];
    bn += tot_n[w];
    bt += tot_t[w];
    btt += tot_tt[w];
  }
#pragma unroll
  for (int trip = 0; trip < kFitTrips; ++trip) {
    const int at = (wave * kFitTrips + trip) * rg::kWave + lane + 1;  // 1 .. 1024 <= kFitSpan + 2
    p_q[at] = bq + q_[trip];
    p_tq[at] = btq + tq_[trip];
    p_n[at] = bn + n_[trip];
    p_t[at] = bt + t_[trip];
    p_tt[at] = btt + tt_[trip];
  }
  if (threadIdx.x == 0) {
    p_q[0] = 0;
    p_tq[0] = 0;
    p_n[0] = 0;
    p_t[0] = 0;
    p_tt[0] = 0;
  }
  __syncthreads();

#pragma unroll
  for (int r = 0; r < kFitTile / rg::kBlock; ++r) {
    const int c = kHalo + r * rg::kBlock + (int)threadIdx.x;          // the entry of this lane's gate
    const int g = g0 + c;
    if (g >= G) continue;
    int L = win.half[0];
    if (dbz) {
      const float z = dbz[in_row + g];                                // a NaN satisfies no comparison: class 0
#pragma unroll
      for (int k = 0; k < RG_PHASE_MAX_CLASSES - 1; ++k) L = z >= win.edge[k] ? win.half[k + 1] : L;   // the edges ascend
    }
    // entries c - L .. c + L: inside the span by construction; those outside the ray are invalid, which clips the window
    const int lo = c - L, hi = c + L + 1;
    const long long N = p_n[hi] - p_n[lo], St = p_t[hi] - p_t[lo], Stt = p_tt[hi] - p_tt[lo];
    const long long Sq = p_q[hi] - p_q[lo], Stq = p_tq[hi] - p_tq[lo];
    const long long Sj = St - (long long)c * N, Sjj = Stt - 2ll * c * St + (long long)c * c * N, Sjq = Stq - (long long)c * Sq;
    const long long den = N * Sjj - Sj * Sj, num = N * Sjq - Sj * Sq;
    const bool centre = p_n[c + 1] - p_n[c] != 0;
    const bool defined = N >= min_valid && den > 0 && (!centre_only || centre);
    float out_k = rg::bits_f32(kNaNBits), out_p = rg::bits_f32(kNaNBits);
    if (defined) {
      const double s = (double)num / (double)den;
      out_k = (float)(s * scale);
      out_p = (float)((((double)Sq - s * (double)Sj) / (double)N) / 65536.0);
    }
    if (kdp) kdp[in_row + g] = out_k;
    if (phi_s) phi_s[in_row + g] = out_p;
    if (count) count[in_row + g] = (uint16_t)N;
  }
}

// ---- attenuation -------------------------------------------------------------------------------------------------------------
// dbz / dbz_out and zdr / zdr_out may be the same arrays: a lane reads its gate before it writes it.
__global__ __launch_bounds__(rg::kBlock) void attenuation_kernel(const float* __restrict__ phi_s, const float* __restrict__ phi0, int R,
                                                                 int G, double alpha, double beta, float cap, const float* dbz,
                                                                 const float* zdr, float* dbz_out, float* zdr_out,
                                                                 float* __restrict__ pia, float* __restrict__ dphi) {
  const int lane = threadIdx.x % rg::kWave;
  const long row = (long)blockIdx.x * kWavesPerBlock + threadIdx.x / rg::kWave;
  if (row >= R) return;                                                               // the whole wavefront
  const size_t in_row = (size_t)row * (size_t)G;
  float origin = phi0 ? phi0[row] : rg::bits_f32(kNaNBits);                           // wave-uniform
  bool has_origin = !isnan(origin);
  float carry = 0.0f;                                                                 // max(+0, every e so far)
  for (int x0 = 0; x0 < G; x0 += rg::kWave) {
    const int x = x0 + lane;
    const bool in = x < G;
    float v = rg::bits_f32(kNaNBits);
    if (in) v = phi_s[in_row + x];
    if (!has_origin) {
      const unsigned long long hit = __ballot(!isnan(v));
      if (hit) {
        origin = __shfl(v, __builtin_ctzll(hit));
        has_origin = true;
      }
    }
    const float e = v - origin;                       // NaN without an origin, for a NaN phi_s, or inf - inf
    float m = e > 0.0f ? e : 0.0f;                    // +0 for whatever is not above 0: max is exact from here on
#pragma unroll
    for (int s = 1; s < rg::kWave; s <<= 1) {
      const float t = __shfl_up(m, s);
      if (lane >= s) m = t > m ? t : m;
    }
    m = carry > m ? carry : m;
    carry = __shfl(m, rg::kWave - 1);
    if (in) {
      const float capped = m < cap ? m : cap;
      const float add = (float)(alpha * (double)capped);
      if (dphi) dphi[in_row + x] = capped;
      if (pia) pia[in_row + x] = add;
      dbz_out[in_row + x] = dbz[in_row + x] + add;
      if (zdr_out) zdr_out[in_row + x] = zdr[in_row + x] + (float)(beta * (double)capped);
    }
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
struct Span {
  const void* p;
  int64_t bytes;
  const char* name;
};

int check_rays(const char* who, int32_t R, int32_t G) {
  RG_REQUIRE(R >= 1, RG_EINVAL, "%s: R must be at least 1, got %d", who, R);
  RG_REQUIRE(G >= 0 && G <= RG_PHASE_MAX_GATES, RG_EINVAL, "%s: G must lie in 0 .. %d, got %d", who, RG_PHASE_MAX_GATES, G);
  RG_REQUIRE((int64_t)R * G < ((int64_t)1 << 31), RG_EINVAL, "%s: R * G must stay below 2^31, got %d x %d", who, R, G);
  return RG_OK;
}

// one launch holds fewer than 2^32 work-items: the header's limit on the workgroups of a call
int check_workgroups(const char* who, int64_t workgroups, int32_t R, int32_t G) {
  RG_REQUIRE(workgroups <= RG_PHASE_MAX_WORKGROUPS, RG_EINVAL, "%s: %d rays of %d gates take %lld workgroups, one launch holds %d", who,
             R, G, (long long)workgroups, RG_PHASE_MAX_WORKGROUPS);
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

int64_t ray_blocks(int32_t R) { return ((int64_t)R + kWavesPerBlock - 1) / kWavesPerBlock; }

}  // namespace

extern "C" int rg_phidp_unfold_f32(const float* phidp, const uint8_t* mask, int32_t R, int32_t G, double wrap, float* out,
                                   int32_t* folds, rg_stream_t stream) {
  const char* who = "rg_phidp_unfold_f32";
  RG_REQUIRE(phidp && out, RG_EINVAL, "%s: null pointer", who);
  int status = check_rays(who, R, G);
  if (status == RG_OK) status = check_workgroups(who, ray_blocks(R), R, G);
  if (status != RG_OK) return status;
  const float half = (float)(0.5 * wrap);
  RG_REQUIRE(isfinite(wrap) && wrap > 0.0 && isfinite(half) && half > 0.0f, RG_EINVAL,
             "%s: wrap must be finite and positive with a finite positive float32 half, got %g", who, wrap);
  const int64_t n = (int64_t)R * G;
  const Span in[] = {{phidp, n * 4, "phidp"}, {mask, n, "mask"}};
  const Span outs[] = {{out, n * 4, "out"}, {folds, n * 4, "folds"}};
  const int same[] = {0, -1};
  status = check_overlaps(who, in, 2, outs, same, 2);
  if (status != RG_OK) return status;
  if (G == 0) return RG_OK;
  hipLaunchKernelGGL(unfold_kernel, dim3((unsigned)ray_blocks(R)), dim3(rg::kBlock), 0, (hipStream_t)stream, phidp, mask, R, G, wrap, half, out,
                     folds);
  return rg::check_launch(who);
}

extern "C" int rg_phidp_fit_f32(const float* phi, int32_t R, int32_t G, const float* dbz, const double* edges_host,
                                const int32_t* half_windows_host, int32_t n_classes, int32_t min_valid, int32_t centre_only,
                                double scale, float* kdp, float* phi_s, uint16_t* count, rg_stream_t stream) {
  const char* who = "rg_phidp_fit_f32";
  RG_REQUIRE(phi && half_windows_host, RG_EINVAL, "%s: null pointer", who);
  RG_REQUIRE(kdp || phi_s, RG_EINVAL, "%s: kdp and phi_s are both NULL", who);
  int status = check_rays(who, R, G);
  const int tiles = (G + kFitTile - 1) / kFitTile;
  if (status == RG_OK) status = check_workgroups(who, (int64_t)R * tiles, R, G);
  if (status != RG_OK) return status;
  RG_REQUIRE(n_classes >= 1 && n_classes <= RG_PHASE_MAX_CLASSES, RG_EINVAL, "%s: n_classes must lie in 1 .. %d, got %d", who,
             RG_PHASE_MAX_CLASSES, n_classes);
  RG_REQUIRE(edges_host || n_classes == 1, RG_EINVAL, "%s: null pointer", who);
  Windows win;
  for (int k = 0; k < RG_PHASE_MAX_CLASSES; ++k) {
    win.half[k] = k < n_classes ? half_windows_host[k] : half_windows_host[n_classes - 1];
    RG_REQUIRE(win.half[k] >= 1 && win.half[k] <= RG_PHASE_MAX_HALF_WINDOW, RG_EINVAL, "%s: half-window %d must lie in 1 .. %d, got %d",
               who, k, RG_PHASE_MAX_HALF_WINDOW, win.half[k]);
  }
  for (int k = 0; k < RG_PHASE_MAX_CLASSES - 1; ++k) {
    win.edge[k] = INFINITY;
    if (k >= n_classes - 1) continue;
    RG_REQUIRE(isfinite(edges_host[k]), RG_EINVAL, "%s: edge %d is not finite", who, k);
    RG_REQUIRE(k == 0 || edges_host[k] >= edges_host[k - 1], RG_EINVAL, "%s: the edges must ascend, edge %d does not", who, k);
    win.edge[k] = (float)edges_host[k];
  }
  RG_REQUIRE(min_valid >= 2 && min_valid <= 2 * RG_PHASE_MAX_HALF_WINDOW + 1, RG_EINVAL, "%s: min_valid must lie in 2 .. %d, got %d",
             who, 2 * RG_PHASE_MAX_HALF_WINDOW + 1, min_valid);
  RG_REQUIRE(isfinite(scale), RG_EINVAL, "%s: scale is not finite", who);
  const int64_t n = (int64_t)R * G;
  const Span in[] = {{phi, n * 4, "phi"}, {dbz, n * 4, "dbz"}};
  const Span outs[] = {{kdp, n * 4, "kdp"}, {phi_s, n * 4, "phi_s"}, {count, n * 2, "count"}};
  const int same[] = {-1, -1, -1};
  status = check_overlaps(who, in, 2, outs, same, 3);
  if (status != RG_OK) return status;
  if (G == 0) return RG_OK;
  hipLaunchKernelGGL(fit_kernel, dim3((unsigned)((int64_t)R * tiles)), dim3(rg::kBlock), 0, (hipStream_t)stream, phi, G, tiles, dbz,
                     win, min_valid, centre_only, scale, kdp, phi_s, count);
  return rg::check_launch(who);
}

extern "C" int rg_attenuation_phidp_f32(const float* phi_s, const float* phi0, int32_t R, int32_t G, double alpha, double beta,
                                        double max_dphi, const float* dbz, const float* zdr, float* dbz_out, float* zdr_out,
                                        float* pia, float* dphi, rg_stream_t stream) {
  const char* who = "rg_attenuation_phidp_f32";
  RG_REQUIRE(phi_s && dbz && dbz_out, RG_EINVAL, "%s: null pointer", who);
  RG_REQUIRE((zdr == nullptr) == (zdr_out == nullptr), RG_EINVAL, "%s: zdr and zdr_out come together or not at all", who);
  int status = check_rays(who, R, G);
  if (status == RG_OK) status = check_workgroups(who, ray_blocks(R), R, G);
  if (status != RG_OK) return status;
  RG_REQUIRE(isfinite(alpha) && alpha >= 0.0 && isfinite(beta) && beta >= 0.0, RG_EINVAL,
             "%s: alpha and beta must be finite and not negative, got %g and %g", who, alpha, beta);
  const float cap = (float)max_dphi;
  RG_REQUIRE(isfinite(max_dphi) && cap > 0.0f, RG_EINVAL, "%s: max_dphi must be finite and positive in float32, got %g", who, max_dphi);
  const int64_t n = (int64_t)R * G;
  const Span in[] = {{phi_s, n * 4, "phi_s"}, {phi0, (int64_t)R * 4, "phi0"}, {dbz, n * 4, "dbz"}, {zdr, n * 4, "zdr"}};
  const Span outs[] = {{dbz_out, n * 4, "dbz_out"}, {zdr_out, n * 4, "zdr_out"}, {pia, n * 4, "pia"}, {dphi, n * 4, "dphi"}};
  const int same[] = {2, 3, -1, -1};
  status = check_overlaps(who, in, 4, outs, same, 4);
  if (status != RG_OK) return status;
  if (G == 0) return RG_OK;
  hipLaunchKernelGGL(attenuation_kernel, dim3((unsigned)ray_blocks(R)), dim3(rg::kBlock), 0, (hipStream_t)stream, phi_s, phi0, R, G, alpha, beta,
                     cap, dbz, zdr, dbz_out, zdr_out, pia, dphi);
  return rg::check_launch(who);
}
