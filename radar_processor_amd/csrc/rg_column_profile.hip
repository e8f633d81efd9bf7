// K5  column profile: echo-top / echo-base heights at up to RG_MAX_PROFILE_THRESHOLDS reflectivity thresholds and the
// vertically integrated liquid (Greene & Clark) of every (y, x) column, in ONE bottom-to-top walk of the stored grid.
// Build-defined (the reference has no such product); the contract is in include/radargrid_hip.h.
//
// Roofline: the echo heights are HBM streaming like K3 -- 4*(z_hi-z_lo+1)*Vxy bytes read, 4*Vxy written per plane, a
// handful of compares and selects per level.  VIL is not: it evaluates a float64 exp10, log2 and exp2 per voxel, which
// outweighs the 4 bytes the voxel costs to read (quotes the measured times).
//
// Mapping (K3's): a lane owns VEC consecutive columns (VEC = 4 -> one dwordx4 per level; VEC = 1 for unaligned planes, for
// n_xy % 4 != 0 and for every launch with VIL, see launch()) and walks the levels of the
// window in order -- never split over lanes: the float64 VIL sum has a fixed order.  Levels are loaded kUnroll at a
// time, ahead of the arithmetic, so that a wave keeps several KiB in flight.  Per column and threshold the walk keeps
//   top:   the highest level k seen so far with g[k] >= T, g[k], and g[k+1] once the walk reaches it (NaN until then, so
//          a crossing at the top of the window has a non-finite neighbour and falls to the level height by itself);
//   base:  the first such level, g[k] and g[k-1] (the previous level's value; NaN at the bottom of the window).
// The kernel is a template on what is asked for: a top-only, one-threshold launch carries three registers per column
// and no transcendental.
#include <float.h>
#include <math.h>

#include "rg_common.hpp"

namespace {

constexpr int kUnroll = 4;   // levels loaded ahead of the arithmetic

struct ProfileArgs {
  double t[RG_MAX_PROFILE_THRESHOLDS];   // thresholds, read on the host
  float t_up[RG_MAX_PROFILE_THRESHOLDS]; // the smallest float32 >= t: for a float32 g, (double)g >= t exactly when g >= t_up
  double vil_max;
};

template <int NT, bool TOP, bool BASE, bool VIL, bool LINEAR>
struct ColumnWalk {
  static constexpr int N = NT > 0 ? NT : 1;
  int k_top[N];
  float g_top[N], g_above[N];
  int k_base[N];
  float g_base[N], g_below[N];
  float prev;     // value of the level below (NaN below the window)
  double sum, q_prev;
  bool any;

  __device__ __forceinline__ void init() {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      k_top[i] = k_base[i] = -2;
      g_top[i] = g_above[i] = g_base[i] = g_below[i] = __builtin_nanf("");
    }
    prev = __builtin_nanf("");
    sum = 0.0; q_prev = 0.0; any = false;
  }

  // level z of the window z_lo ..: value v; dz = z_levels[z] - z_levels[z - 1] (unused at z_lo)
  __device__ __forceinline__ void step(const ProfileArgs& a, int z, int z_lo, float v, double dz) {
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const bool hit = v >= a.t_up[i];                   // (double)v >= t; NaN never reaches a threshold
      if constexpr (TOP) {
        if (hit) {
          k_top[i] = z;
          if constexpr (LINEAR) { g_top[i] = v; g_above[i] = __builtin_nanf(""); }
        } else if constexpr (LINEAR) {
          if (k_top[i] == z - 1) g_above[i] = v;
        }
      }
      if constexpr (BASE) {
        if (hit && k_base[i] < 0) {
          k_base[i] = z;
          if constexpr (LINEAR) { g_base[i] = v; g_below[i] = prev; }
        }
      }
    }
    if constexpr (BASE && LINEAR) prev = v;
    if constexpr (VIL) {
      const bool nan = isnan(v);
      const double vd = (double)v;
      const double capped = vd < a.vil_max ? vd : a.vil_max;
      const double q = nan ? 0.0 : exp10(capped / 10.0);
      // x^(4/7) as exp2(y), y = 4/7 * log2(x), not pow(): measured on the bench grid with four columns per lane, VIL alone
      // took 0.78 ms this way and 1.13 ms with pow() (profiles/column_profile_timing.json: `vil_four_columns_build` against
      // `earlier_build`).  The rounding of y enters the result as
      // |y| * 2^-53 * ln 2 -- ~1e-15 relative for |y| <= 16, i.e. up to 80 dBZ -- far below the plane's float32 rounding
      if (z > z_lo) sum = sum + exp2((4.0 / 7.0) * log2((q_prev + q) / 2.0)) * dz;
      q_prev = q;
      any = any || !nan;
    }
  }

  // z_levels[clamp(k, z_lo, z_hi)]: every index formed here stays inside the window
  static __device__ __forceinline__ double level(const double* __restrict__ zl, int k, int z_lo, int z_hi) {
    return zl[k < z_lo ? z_lo : (k > z_hi ? z_hi : k)];
  }

  __device__ __forceinline__ float top(const ProfileArgs& a, int i, const double* __restrict__ zl, int z_lo, int z_hi) const {
    const int k = k_top[i];
    if (k < 0) return __builtin_nanf("");
    const double zk = level(zl, k, z_lo, z_hi);
    if constexpr (LINEAR) {
      if (isfinite(g_top[i]) && isfinite(g_above[i])) {
        const double zn = level(zl, k + 1, z_lo, z_hi);
        const double gk = (double)g_top[i];
        return (float)(zk + ((gk - a.t[i]) / (gk - (double)g_above[i])) * (zn - zk));
      }
    }
    return (float)zk;
  }

  __device__ __forceinline__ float base(const ProfileArgs& a, int i, const double* __restrict__ zl, int z_lo, int z_hi) const {
    const int k = k_base[i];
    if (k < 0) return __builtin_nanf("");
    const double zk = level(zl, k, z_lo, z_hi);
    if constexpr (LINEAR) {
      if (isfinite(g_base[i]) && isfinite(g_below[i])) {
        const double zp = level(zl, k - 1, z_lo, z_hi);
        const double gk = (double)g_base[i];
        return (float)(zk - ((gk - a.t[i]) / (gk - (double)g_below[i])) * (zk - zp));
      }
    }
    return (float)zk;
  }

  __device__ __forceinline__ float vil() const { return any ? (float)(3.44e-6 * sum) : __builtin_nanf(""); }
};

template <int VEC>
__device__ __forceinline__ void load_level(const float* __restrict__ grid, long n_xy, int z, long c0, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 q = *reinterpret_cast<const float4*>(grid + (size_t)z * n_xy + c0);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = grid[(size_t)z * n_xy + c0];
  }
}

template <int VEC>
__device__ __forceinline__ void store_plane(float* __restrict__ plane, long c0, const float (&r)[VEC]) {
  if constexpr (VEC == 4) *reinterpret_cast<float4*>(plane + c0) = make_float4(r[0], r[1], r[2], r[3]);
  else plane[c0] = r[0];
}

template <int NT, bool TOP, bool BASE, bool VIL, bool LINEAR, int VEC>
__global__ __launch_bounds__(rg::kBlock) void column_profile_kernel(const float* __restrict__ grid, long n_xy, int z_lo, int z_hi,
                                                                    const double* __restrict__ zl, ProfileArgs a,
                                                                    float* __restrict__ out_top, float* __restrict__ out_base,
                                                                    float* __restrict__ out_vil) {
  const long c0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * VEC;
  if (c0 >= n_xy) return;
  ColumnWalk<NT, TOP, BASE, VIL, LINEAR> col[VEC];
#pragma unroll
  for (int c = 0; c < VEC; ++c) col[c].init();

  int z = z_lo;
  for (; z + kUnroll - 1 <= z_hi; z += kUnroll) {
    float v[kUnroll][VEC];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) load_level<VEC>(grid, n_xy, z + u, c0, v[u]);
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const double dz = VIL && z + u > z_lo ? zl[z + u] - zl[z + u - 1] : 0.0;
#pragma unroll
      for (int c = 0; c < VEC; ++c) col[c].step(a, z + u, z_lo, v[u][c], dz);
    }
  }
  for (; z <= z_hi; ++z) {
    float v[VEC];
    load_level<VEC>(grid, n_xy, z, c0, v);
    const double dz = VIL && z > z_lo ? zl[z] - zl[z - 1] : 0.0;
#pragma unroll
    for (int c = 0; c < VEC; ++c) col[c].step(a, z, z_lo, v[c], dz);
  }

  float r[VEC];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    if constexpr (TOP) {
#pragma unroll
      for (int c = 0; c < VEC; ++c) r[c] = col[c].top(a, i, zl, z_lo, z_hi);
      store_plane<VEC>(out_top + (size_t)i * n_xy, c0, r);
    }
    if constexpr (BASE) {
#pragma unroll
      for (int c = 0; c < VEC; ++c) r[c] = col[c].base(a, i, zl, z_lo, z_hi);
      store_plane<VEC>(out_base + (size_t)i * n_xy, c0, r);
    }
  }
  if constexpr (VIL) {
#pragma unroll
    for (int c = 0; c < VEC; ++c) r[c] = col[c].vil();
    store_plane<VEC>(out_vil, c0, r);
  }
}

struct Launch {
  const float* grid; long n_xy; int z_lo, z_hi; const double* zl; ProfileArgs a;
  float *out_top, *out_base, *out_vil; bool vec; hipStream_t s;
};

template <int NT, bool TOP, bool BASE, bool VIL, bool LINEAR>
int launch(const Launch& l) {
  // A launch with VIL always takes one column per lane: four columns' worth of float64 exp10 / log2 / exp2 temporaries
  // cost it occupancy (93-192 VGPRs against 65-98) and it is bound by that arithmetic, not by the width of its loads --
  // measured on the bench grid, VIL alone 0.72 against 0.78 ms, four thresholds top + base + VIL 0.89 against 1.07 ms
  // (profiles/column_profile_timing.json: `vil_1col` / `top4_base4_vil_1col` against `vil` / `top4_base4_vil` of its
  // `vil_four_columns_build`), so the four-column VIL instantiations are not compiled.
  const bool vec = l.vec && !VIL;
  const long groups = vec ? l.n_xy / 4 : l.n_xy;
  const dim3 g((unsigned)((groups + rg::kBlock - 1) / rg::kBlock)), b(rg::kBlock);
  if constexpr (!VIL) {
    if (vec) {
      hipLaunchKernelGGL((column_profile_kernel<NT, TOP, BASE, VIL, LINEAR, 4>), g, b, 0, l.s, l.grid, l.n_xy, l.z_lo, l.z_hi,
                         l.zl, l.a, l.out_top, l.out_base, l.out_vil);
      return rg::check_launch("rg_column_profile_f32");
    }
  }
  hipLaunchKernelGGL((column_profile_kernel<NT, TOP, BASE, VIL, LINEAR, 1>), g, b, 0, l.s, l.grid, l.n_xy, l.z_lo, l.z_hi, l.zl,
                     l.a, l.out_top, l.out_base, l.out_vil);
  return rg::check_launch("rg_column_profile_f32");
}

// the smallest float32 >= t (t finite)
float round_up_f32(double t) {
  if (t > (double)FLT_MAX) return INFINITY;
  if (t < -(double)FLT_MAX) return -FLT_MAX;
  const float f = (float)t;
  return (double)f < t ? nextafterf(f, INFINITY) : f;
}

template <class F>
int dispatch_bool(bool v, F&& f) {
  return v ? f(std::true_type{}) : f(std::false_type{});
}

// n_thresholds 1 .. RG_MAX_PROFILE_THRESHOLDS (checked by the caller) -> f(int_c<NT>)
template <int NT = 1, class F>
int dispatch_thresholds(int nt, F&& f) {
  if constexpr (NT < RG_MAX_PROFILE_THRESHOLDS) {
    if (nt != NT) return dispatch_thresholds<NT + 1>(nt, f);
  }
  return f(rg::int_c<NT>{});
}

}  // namespace

extern "C" int rg_column_profile_f32(const float* grid, int32_t nz, int64_t n_xy, int32_t z_lo, int32_t z_hi,
                                     const double* z_levels, const double* thresholds_host, int32_t n_thresholds,
                                     int32_t linear, float* out_top, float* out_base, double vil_max_dbz, float* out_vil,
                                     rg_stream_t stream) {
  const char* me = "rg_column_profile_f32";
  RG_REQUIRE(grid && z_levels, RG_EINVAL, "%s: null pointer", me);
  RG_REQUIRE(out_top || out_base || out_vil, RG_EINVAL, "%s: nothing to produce", me);
  RG_REQUIRE(nz >= 1 && n_xy >= 0, RG_EINVAL, "%s: bad shape nz=%d n_xy=%lld", me, nz, (long long)n_xy);
  RG_REQUIRE(n_thresholds >= 0 && n_thresholds <= RG_MAX_PROFILE_THRESHOLDS, RG_EINVAL, "%s: %d thresholds (0..%d per call)", me,
             n_thresholds, RG_MAX_PROFILE_THRESHOLDS);
  RG_REQUIRE(n_thresholds > 0 || (!out_top && !out_base), RG_EINVAL, "%s: echo top / base without a threshold", me);
  RG_REQUIRE(n_thresholds == 0 || thresholds_host, RG_EINVAL, "%s: null thresholds", me);
  ProfileArgs a;
  for (int i = 0; i < RG_MAX_PROFILE_THRESHOLDS; ++i) {
    a.t[i] = i < n_thresholds ? thresholds_host[i] : 0.0;
    RG_REQUIRE(std::isfinite(a.t[i]), RG_EINVAL, "%s: threshold %d is not finite", me, i);
    a.t_up[i] = round_up_f32(a.t[i]);
  }
  RG_REQUIRE(std::isfinite(vil_max_dbz), RG_EINVAL, "%s: vil_max_dbz is not finite", me);
  a.vil_max = vil_max_dbz;
  RG_REQUIRE(z_lo >= 0 && z_hi < nz && z_lo <= z_hi, RG_EINVAL, "%s: level window [%d,%d] outside 0..%d or empty", me, z_lo, z_hi,
             nz - 1);
  if (n_xy == 0) return RG_OK;
  Launch l;
  l.grid = grid; l.n_xy = (long)n_xy; l.z_lo = z_lo; l.z_hi = z_hi; l.zl = z_levels; l.a = a;
  l.out_top = out_top; l.out_base = out_base; l.out_vil = out_vil; l.s = (hipStream_t)stream;
  l.vec = (n_xy % 4 == 0) && rg::aligned16(grid) && (!out_top || rg::aligned16(out_top)) &&
          (!out_base || rg::aligned16(out_base)) && (!out_vil || rg::aligned16(out_vil));
  RG_REQUIRE((n_xy + rg::kBlock - 1) / rg::kBlock <= 0x7FFFFFFFLL, RG_EUNSUPPORTED,
             "%s: %lld columns exceed one launch", me, (long long)n_xy);
  const bool top = out_top != nullptr, base = out_base != nullptr, vil = out_vil != nullptr;
  if (!top && !base) return launch<0, false, false, true, false>(l);   // thresholds without a plane of theirs: VIL alone
  return dispatch_thresholds(n_thresholds, [&](auto nt) {
    return dispatch_bool(vil, [&](auto v) {
      return dispatch_bool(linear != 0, [&](auto lin) {
        constexpr int NT = decltype(nt)::value;
        constexpr bool V = decltype(v)::value, L = decltype(lin)::value;
        if (top && base) return launch<NT, true, true, V, L>(l);
        if (top) return launch<NT, true, false, V, L>(l);
        return launch<NT, false, true, V, L>(l);
      });
    });
  });
}
