// Texture along the ray and the table-driven fuzzy-logic classifier (include/radargrid_hydro.h).
//
// texture   blockIdx strides over (ray, tile) pairs.  Entry e of a tile's span is gate tile * kTile - kHalo + e; only the entries
//           within L of the tile are loaded, the others (and gates outside the ray, and invalid gates) count nothing.  Each
//           wavefront scans kTrips * 64 consecutive entries with the shuffle ladder -- (valid, q, q * q), the count by ballot and
//           popcount -- the wavefronts' totals are added before the one write, and prefix index e + 1 holds the sums over the
//           entries 0 .. e.  A lane then takes two prefix reads per sum for each of its kTile / 256 gates.  Consecutive lanes read
//           consecutive words: no bank conflict anywhere.
// classify  the cell table goes to LDS once per workgroup (dynamic LDS: 48 bytes per cell), then the workgroup strides over the
//           gates, a lane per gate.  The kernel is instantiated per V, so the V values of a gate are registers and the loop
//           over the variables is unrolled; weights, kinds and edges are read from the argument block with uniform indices
//           (scalar loads).  A lane reads the six doubles of a cell of ITS bin: neighbouring gates mostly share a bin, and equal
//           addresses broadcast.
#include <math.h>

#include <atomic>

#include "radargrid_hydro.h"
#include "rg_common.hpp"

namespace {

constexpr uint32_t kQuietNaN = 0x7FC00000u;

// ---- 1  texture ------------------------------------------------------------------------------------------------------------------
constexpr int kHalo = RG_HYDRO_MAX_HALF_GATES;                // 63
constexpr int kTile = RG_HYDRO_TEXTURE_TILE;                  // 512
constexpr int kSpan = kTile + 2 * kHalo;                      // 638 entries are scanned for a tile
constexpr int kWaves = rg::kBlock / rg::kWave;                // 4
constexpr int kTrips = (kSpan + rg::kBlock - 1) / rg::kBlock; // 3 trips of 64 entries per wavefront
constexpr int kSlots = kTrips * rg::kBlock + 1;               // prefix indices 0 .. 768
constexpr long kTextureGrid = 1l << 20;                       // workgroups of one launch at most; they stride over the tiles
static_assert(kTile % rg::kBlock == 0, "every lane takes kTile / 256 gates");
static_assert((long long)kSpan << (2 * (13 + RG_HYDRO_TEXTURE_SHIFT)) < (1ll << 56), "the prefix of q * q fits");

__device__ __forceinline__ unsigned long long lanes_upto(int lane) { return lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull; }

__global__ __launch_bounds__(rg::kBlock) void texture_kernel(const float* __restrict__ x, const uint8_t* __restrict__ mask, int G,
                                                             int tiles, long total, int L, int min_valid, int centre_only,
                                                             float* __restrict__ sd, float* __restrict__ mean,
                                                             uint16_t* __restrict__ count) {
  __shared__ long long p_q[kSlots], p_qq[kSlots];
  __shared__ int p_n[kSlots];
  __shared__ long long tot_q[kWaves], tot_qq[kWaves];
  __shared__ int tot_n[kWaves];
  const int lane = threadIdx.x % rg::kWave, wave = threadIdx.x / rg::kWave;
  const unsigned long long upto = lanes_upto(lane);
  for (long id = blockIdx.x; id < total; id += gridDim.x) {
    const long ray = id / tiles;
    const int tile = (int)(id - ray * tiles);
    const size_t row = (size_t)ray * (size_t)G;
    const int g0 = tile * kTile - kHalo;                      // the gate of entry 0

    long long q_[kTrips], qq_[kTrips];
    int n_[kTrips];
    long long cq = 0, cqq = 0;
    int cn = 0;
#pragma unroll
    for (int trip = 0; trip < kTrips; ++trip) {
      const int e = (wave * kTrips + trip) * rg::kWave + lane, g = g0 + e;
      long long q = 0;
      bool valid = false;
      if (e >= kHalo - L && e < kHalo + kTile + L && g >= 0 && g < G) {
        const float v = x[row + g];
        valid = fabsf(v) <= (float)RG_HYDRO_MAX_ABS && !(mask && mask[row + g]);   // false for NaN and +-inf
        if (valid) q = llrint(1024.0 * (double)v);
      }
      const unsigned long long hit = __ballot(valid);
      long long qq = q * q;
#pragma unroll
      for (int s = 1; s < rg::kWave; s <<= 1) {
        const long long aq = __shfl_up(q, s), aqq = __shfl_up(qq, s);
        if (lane >= s) {
          q += aq;
          qq += aqq;
        }
      }
      q_[trip] = cq + q;
      qq_[trip] = cqq + qq;
      n_[trip] = cn + __builtin_popcountll(hit & upto);
      cq += __shfl(q, rg::kWave - 1);
      cqq += __shfl(qq, rg::kWave - 1);
      cn += __builtin_popcountll(hit);
    }
    if (lane == 0) {
      tot_q[wave] = cq;
      tot_qq[wave] = cqq;
      tot_n[wave] = cn;
    }
    __syncthreads();
    long long bq = 0, bqq = 0;                                // the wavefronts before this one
    int bn = 0;
    for (int w = 0; w < wave; ++w) {
      bq += tot_q[w];
      bqq += tot_qq[w];
      bn += tot_n[w];
    }
#pragma unroll
    for (int trip = 0; trip < kTrips; ++trip) {
      const int at = (wave * kTrips + trip) * rg::kWave + lane + 1;   // 1 .. 768 = kSlots - 1
      p_q[at] = bq + q_[trip];
      p_qq[at] = bqq + qq_[trip];
      p_n[at] = bn + n_[trip];
    }
    if (threadIdx.x == 0) {
      p_q[0] = 0;
      p_qq[0] = 0;
      p_n[0] = 0;
    }
    __syncthreads();

#pragma unroll
    for (int r = 0; r < kTile / rg::kBlock; ++r) {
      const int c = kHalo + r * rg::kBlock + (int)threadIdx.x;        // the entry of this lane's gate
      const int g = g0 + c;
      if (g >= G) continue;
      const int lo = c - L, hi = c + L + 1;                           // 0 <= lo, hi <= kSpan: inside the prefixes
      const long long N = p_n[hi] - p_n[lo], Sq = p_q[hi] - p_q[lo], Sqq = p_qq[hi] - p_qq[lo];
      const bool centre = p_n[c + 1] - p_n[c] != 0;
      const bool defined = N >= min_valid && (!centre_only || centre);
      float out_sd = rg::bits_f32(kQuietNaN), out_mean = rg::bits_f32(kQuietNaN);
      if (defined) {
        const long long D = N * Sqq - Sq * Sq;
        out_sd = (float)((sqrt((double)D) / (double)N) / 1024.0);
        out_mean = (float)(((double)Sq / (double)N) / 1024.0);
      }
      if (sd) sd[row + g] = out_sd;
      if (mean) mean[row + g] = out_mean;
      if (count) count[row + g] = (uint16_t)N;
    }
    __syncthreads();                                                  // the prefixes are rewritten by the next tile
  }
}

// ---- 2  classifier ---------------------------------------------------------------------------------------------------------------
constexpr int kCellDoubles = 6;
constexpr int kComputeUnits = 256;                            // the whole MI355X; what compute_units() falls back to
constexpr int kLdsPerCu = 160 * 1024;                         // gfx950

struct ClassifyArgs {
  const float* var[RG_HYDRO_MAX_VARS];
  double weight[RG_HYDRO_MAX_CLASSES * RG_HYDRO_MAX_VARS];    // [C][V], packed with pitch V
  double min_score;
  float edge[RG_HYDRO_MAX_BINS - 1];                          // (float)edges_host[k]
  int n_edges;
  int multiplicative_bits, per_sweep_bits, required_bits;
  int cond_var;
  int C;
  int rays_per_sweep;
  int G;
  long n_gates;
  int n_cells;
};

template <int V>
__global__ __launch_bounds__(rg::kBlock) void classify_kernel(const ClassifyArgs a, const uint8_t* __restrict__ mask,
                                                              const double* __restrict__ cells, uint8_t* __restrict__ cls,
                                                              float* __restrict__ score, uint8_t* __restrict__ second) {
  extern __shared__ double s_cells[];
  for (int i = threadIdx.x; i < a.n_cells * kCellDoubles; i += rg::kBlock) s_cells[i] = cells[i];
  __syncthreads();
  const long step = (long)gridDim.x * rg::kBlock;
  for (long at = (long)blockIdx.x * rg::kBlock + threadIdx.x; at < a.n_gates; at += step) {
    const long ray = at / a.G;
    const int g = (int)(at - ray * a.G);
    const long sweep_at = (ray / a.rays_per_sweep) * a.G + g;
    float value[V];
    bool classified = !(mask && mask[at]);
    int bin = 0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      value[v] = a.var[v][(a.per_sweep_bits >> v) & 1 ? sweep_at : at];
      const bool present = isfinite(value[v]);
      if (((a.required_bits >> v) & 1) && !present) classified = false;
      if (v == a.cond_var) {
        if (!present) classified = false;
        for (int k = 0; k < a.n_edges; ++k) bin += value[v] >= a.edge[k] ? 1 : 0;
      }
    }
    double best = -1.0, next = -1.0;
    int k1 = -1, k2 = -1;
    if (classified) {
      const double* cell = s_cells + (size_t)bin * a.C * V * kCellDoubles;
      for (int c = 0; c < a.C; ++c) {
        double A = 0.0, W = 0.0, P = 1.0;
#pragma unroll
        for (int v = 0; v < V; ++v, cell += kCellDoubles) {
          if (!isfinite(value[v])) continue;
          const double x = (double)value[v];
          const double x1 = cell[0], x2 = cell[1], x3 = cell[2], x4 = cell[3];
          double m;
          if (x < x1 || x > x4) {
            m = 0.0;
          } else if (x2 <= x && x <= x3) {
            m = 1.0;
          } else if (x < x2) {
            const double t = (x - x1) * cell[4];
            m = t < 1.0 ? t : 1.0;
          } else {
            const double t = (x4 - x) * cell[5];
            m = t < 1.0 ? t : 1.0;
          }
          if ((a.multiplicative_bits >> v) & 1) {
            P *= m;
          } else {
            const double w = a.weight[c * V + v];
            A += w * m;
            W += w;
          }
        }
        const double s = (W > 0.0 ? A / W : 0.0) * P;
        if (s > best) {                                       // strictly: the lowest class among equals stays
          next = best;
          k2 = k1;
          best = s;
          k1 = c;
        } else if (s > next) {
          next = s;
          k2 = c;
        }
      }
    }
    const bool won = k1 >= 0 && best > 0.0 && !(best < a.min_score);
    cls[at] = won ? (uint8_t)(k1 + 1) : (uint8_t)RG_HYDRO_UNCLASSIFIED;
    if (score) score[at] = won ? (float)best : rg::bits_f32(kQuietNaN);
    if (second) second[at] = won ? (uint8_t)(k2 + 1) : (uint8_t)0;
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
struct Span {
  const void* p;
  int64_t bytes;
  const char* name;
};

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// R >= 1, 0 <= G <= RG_PHASE_MAX_GATES and R * G < 2^31
int check_rays(const char* who, int32_t R, int32_t G) {
  RG_REQUIRE(R >= 1, RG_EINVAL, "%s: R must be at least 1, got %d", who, R);
  RG_REQUIRE(G >= 0 && G <= RG_PHASE_MAX_GATES, RG_EINVAL, "%s: G must lie in 0 .. %d, got %d", who, RG_PHASE_MAX_GATES, G);
  RG_REQUIRE((int64_t)R * G < ((int64_t)1 << 31), RG_EINVAL, "%s: %d rays of %d gates are 2^31 gates or more", who, R, G);
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

// The compute units of the current device, asked of the runtime once per device and kept (a partition of the part has fewer
// than the whole one's 256).  Only the number of workgroups of a launch depends on it, never a result.
int compute_units() {
  constexpr int kMaxDevices = 64;
  static std::atomic<int> cached[kMaxDevices];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return kComputeUnits;
  int n = cached[dev].load(std::memory_order_relaxed);
  if (n == 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = kComputeUnits;
    cached[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

}  // namespace

extern "C" int rg_polar_texture_f32(const float* x, const uint8_t* mask, int32_t R, int32_t G, int32_t half_gates, int32_t min_valid,
                                    int32_t centre_only, float* sd, float* mean, uint16_t* count, rg_stream_t stream) {
  const char* who = "rg_polar_texture_f32";
  RG_REQUIRE(x, RG_EINVAL, "%s: null pointer", who);
  RG_REQUIRE(sd || mean, RG_EINVAL, "%s: neither sd nor mean is asked for", who);
  int status = check_rays(who, R, G);
  if (status != RG_OK) return status;
  RG_REQUIRE(half_gates >= 1 && half_gates <= RG_HYDRO_MAX_HALF_GATES, RG_EINVAL, "%s: half_gates must lie in 1 .. %d, got %d", who,
             RG_HYDRO_MAX_HALF_GATES, half_gates);
  RG_REQUIRE(min_valid >= 1 && min_valid <= 2 * RG_HYDRO_MAX_HALF_GATES + 1, RG_EINVAL, "%s: min_valid must lie in 1 .. %d, got %d", who,
             2 * RG_HYDRO_MAX_HALF_GATES + 1, min_valid);
  const int64_t n = (int64_t)R * G;
  const Span in[] = {{x, n * 4, "x"}, {mask, n, "mask"}};
  const Span outs[] = {{sd, n * 4, "sd"}, {mean, n * 4, "mean"}, {count, n * 2, "count"}};
  status = check_overlaps(who, in, 2, outs, 3);
  if (status != RG_OK) return status;
  if (G == 0) return RG_OK;
  const int tiles = (G + kTile - 1) / kTile;
  const long total = (long)R * tiles;                          // <= R * G < 2^31
  const long blocks = total < kTextureGrid ? total : kTextureGrid;
  hipLaunchKernelGGL(texture_kernel, dim3((unsigned)blocks), dim3(rg::kBlock), 0, (hipStream_t)stream, x, mask, G, tiles, total,
                     half_gates, min_valid, centre_only ? 1 : 0, sd, mean, count);
  return rg::check_launch(who);
}

extern "C" int rg_fuzzy_classify_f32(const float* const* vars_host, const int32_t* kind_host, int32_t V, int32_t per_sweep_bits,
                                     int32_t required_bits, int32_t rays_per_sweep, const uint8_t* mask, int32_t R, int32_t G,
                                     int32_t cond_var, const double* edges_host, int32_t B, const double* cells, int32_t C,
                                     const double* weights_host, double min_score, uint8_t* cls, float* score, uint8_t* second,
                                     rg_stream_t stream) {
  const char* who = "rg_fuzzy_classify_f32";
  RG_REQUIRE(vars_host && kind_host && weights_host && cells && cls, RG_EINVAL, "%s: null pointer", who);
  RG_REQUIRE(V >= 1 && V <= RG_HYDRO_MAX_VARS, RG_EINVAL, "%s: V must lie in 1 .. %d, got %d", who, RG_HYDRO_MAX_VARS, V);
  RG_REQUIRE(C >= 1 && C <= RG_HYDRO_MAX_CLASSES, RG_EINVAL, "%s: C must lie in 1 .. %d, got %d", who, RG_HYDRO_MAX_CLASSES, C);
  RG_REQUIRE(B >= 1 && B <= RG_HYDRO_MAX_BINS, RG_EINVAL, "%s: B must lie in 1 .. %d, got %d", who, RG_HYDRO_MAX_BINS, B);
  RG_REQUIRE(B * C * V <= RG_HYDRO_MAX_CELLS, RG_EINVAL, "%s: %d x %d x %d cells are more than %d", who, B, C, V, RG_HYDRO_MAX_CELLS);
  ClassifyArgs a = {};
  for (int v = 0; v < V; ++v) {
    RG_REQUIRE(vars_host[v], RG_EINVAL, "%s: variable %d is a null pointer", who, v);
    RG_REQUIRE(kind_host[v] == 0 || kind_host[v] == 1, RG_EINVAL, "%s: the kind of variable %d must be 0 or 1, got %d", who, v,
               kind_host[v]);
    a.var[v] = vars_host[v];
    a.multiplicative_bits |= kind_host[v] << v;
  }
  RG_REQUIRE(a.multiplicative_bits != (1 << V) - 1, RG_EINVAL, "%s: no variable is additive", who);
  RG_REQUIRE(per_sweep_bits >= 0 && per_sweep_bits < (1 << V) && required_bits >= 0 && required_bits < (1 << V), RG_EINVAL,
             "%s: per_sweep_bits and required_bits must lie in 0 .. %d, got %d and %d", who, (1 << V) - 1, per_sweep_bits,
             required_bits);
  int status = check_rays(who, R, G);
  if (status != RG_OK) return status;
  RG_REQUIRE(rays_per_sweep >= 1 && R % rays_per_sweep == 0, RG_EINVAL, "%s: rays_per_sweep must be at least 1 and divide R = %d, got %d",
             who, R, rays_per_sweep);
  RG_REQUIRE(cond_var >= -1 && cond_var < V, RG_EINVAL, "%s: cond_var must lie in -1 .. %d, got %d", who, V - 1, cond_var);
  RG_REQUIRE(cond_var >= 0 || B == 1, RG_EINVAL, "%s: %d bins without a condition variable", who, B);
  RG_REQUIRE(B == 1 || edges_host, RG_EINVAL, "%s: %d bins without edges", who, B);
  for (int k = 0; k + 1 < B; ++k) {
    RG_REQUIRE(isfinite(edges_host[k]), RG_EINVAL, "%s: edge %d is not finite", who, k);
    RG_REQUIRE(k == 0 || edges_host[k] >= edges_host[k - 1], RG_EINVAL, "%s: the edges descend at edge %d", who, k);
    a.edge[k] = (float)edges_host[k];
  }
  for (int k = 0; k < C * V; ++k) {
    RG_REQUIRE(isfinite(weights_host[k]) && weights_host[k] >= 0.0, RG_EINVAL, "%s: weight %d of class %d must be finite and not negative, got %g",
               who, k % V, k / V, weights_host[k]);
    a.weight[k] = weights_host[k];
  }
  RG_REQUIRE(isfinite(min_score) && min_score >= 0.0, RG_EINVAL, "%s: min_score must be finite and not negative, got %g", who, min_score);
  RG_REQUIRE(aligned_to(cells, 8), RG_EALIGN, "%s: cells must be 8-byte aligned", who);
  const int64_t n = (int64_t)R * G;
  static const char* const kVarNames[RG_HYDRO_MAX_VARS] = {"variable 0", "variable 1", "variable 2", "variable 3",
                                                           "variable 4", "variable 5", "variable 6", "variable 7"};
  Span in[RG_HYDRO_MAX_VARS + 2];
  for (int v = 0; v < V; ++v) in[v] = {vars_host[v], ((per_sweep_bits >> v) & 1 ? n / rays_per_sweep : n) * 4, kVarNames[v]};
  in[V] = {mask, n, "mask"};
  in[V + 1] = {cells, (int64_t)B * C * V * kCellDoubles * 8, "cells"};
  const Span outs[] = {{cls, n, "cls"}, {score, n * 4, "score"}, {second, n, "second"}};
  status = check_overlaps(who, in, V + 2, outs, 3);
  if (status != RG_OK) return status;
  if (G == 0) return RG_OK;
  a.n_edges = B - 1;
  a.per_sweep_bits = per_sweep_bits;
  a.required_bits = required_bits;
  a.cond_var = cond_var;
  a.C = C;
  a.rays_per_sweep = rays_per_sweep;
  a.G = G;
  a.n_gates = (long)n;
  a.n_cells = B * C * V;
  a.min_score = min_score;
  const size_t lds = (size_t)a.n_cells * kCellDoubles * sizeof(double);          // <= 49152
  // as many workgroups as the CUs hold at once (by LDS, eight at most), each staging the table once and striding over the gates
  long resident = kLdsPerCu / (long)lds;
  resident = resident > 8 ? 8 : resident;
  const long most = compute_units() * resident, needed = (long)((n + rg::kBlock - 1) / rg::kBlock);
  const unsigned blocks = (unsigned)(needed < most ? needed : most);
  return rg::dispatch_fields<RG_HYDRO_MAX_VARS>(V, [&](auto nv, auto) {
    hipLaunchKernelGGL((classify_kernel<decltype(nv)::value>), dim3(blocks), dim3(rg::kBlock), lds, (hipStream_t)stream, a, mask, cells,
                       cls, score, second);
    return rg::check_launch(who);
  });
}
