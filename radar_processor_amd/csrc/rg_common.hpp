// Shared helpers for libradargrid_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "radargrid_hip.h"

namespace rg {

void set_error(const char* fmt, ...);

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// [a, a + a_bytes) and [b, b + b_bytes) share a byte
inline bool overlap(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + (uintptr_t)b_bytes && pb < pa + (uintptr_t)a_bytes;
}

// checks the launch that was just enqueued; does not synchronise
inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return RG_ELAUNCH;
  }
  return RG_OK;
}

// every double of an rg_georef is finite (the entry points that take one refuse it otherwise)
inline bool georef_finite(const rg_georef& g) {
  const double m[] = {g.radius, g.lon_from, g.lat_from, g.sin_lat_from, g.cos_lat_from, g.lon_to, g.lat_to,
                      g.sin_lat_to, g.cos_lat_to, g.ox, g.oy};
  for (double v : m)
    if (!__builtin_isfinite(v)) return false;
  return true;
}

constexpr int kWave = 64;        // CDNA4 wavefront
constexpr int kBlock = 256;      // 4 waves per workgroup

// ---- clearing accumulators and scratch on the stream ----
// A kernel, not hipMemsetAsync.  Observed with HIP 7.0 (tests/test_gpu_graph_replay.py; the cause inside the runtime is not
// established): a captured graph zeroes through a memset node on its first replay only; from the second replay on the words
// come out as a repeating 16 bytes of other data, as if the node's fill pattern were read from memory that has been reused.
// A kernel node keeps `value` among its own arguments, so it does not depend on that.
template <int = 0>
__global__ __launch_bounds__(kBlock) void fill_words_kernel(uint32_t* __restrict__ p, long n, uint32_t value) {
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) p[i] = value;
}

// `bytes` (a multiple of 4, below 2^40) at the 4-byte aligned `p` become copies of the 32-bit `value`; enqueues, never waits
inline void fill_words(void* p, int64_t bytes, uint32_t value, hipStream_t s) {
  const long n = (long)(bytes / 4);
  if (n > 0)
    hipLaunchKernelGGL(fill_words_kernel<>, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, static_cast<uint32_t*>(p),
                       n, value);
}

// float32 slots per gate of the packed fields (rg_pack_fields_f32) for a pass of nf fields: the gather is one 4-, 8- or
// 16-byte load, or two of 16
constexpr int stride_for(int nf) { return nf == 1 ? 1 : nf == 2 ? 2 : nf <= 4 ? 4 : 8; }

// ---- run-time value -> template argument: the launchers pass a generic lambda and read the constants off its parameters ----
template <int V>
using int_c = std::integral_constant<int, V>;

// n_fields (1 .. MAXF, checked by the caller) -> f(int_c<NF>, int_c<STRIDE>), STRIDE = stride_for(NF); only 1 .. MAXF are
// instantiated
template <int MAXF = RG_MAX_FIELDS, int NF = 1, class F>
int dispatch_fields(int nf, F&& f) {
  if constexpr (NF < MAXF) {
    if (nf != NF) return dispatch_fields<MAXF, NF + 1>(nf, f);
  }
  return f(int_c<NF>{}, int_c<stride_for(NF)>{});
}

// width of the row pointers -> f(IndT{}), IndT = int64_t or int32_t
template <class F>
int dispatch_index(bool is_i64, F&& f) {
  return is_i64 ? f(int64_t{}) : f(int32_t{});
}

__device__ __forceinline__ uint32_t f32_bits(float v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ float bits_f32(uint32_t v) { return __builtin_bit_cast(float, v); }

// One gather of a gate's packed field slots (layout of rg_pack_fields_f32: float32 [G][STRIDE], STRIDE in {1,2,4,8}).
template <int STRIDE>
__device__ __forceinline__ void load_packed(const float* __restrict__ p, unsigned g, float (&v)[STRIDE]) {
  if constexpr (STRIDE == 1) {
    v[0] = p[g];
  } else if constexpr (STRIDE == 2) {
    const float2 t = reinterpret_cast<const float2*>(p)[g];
    v[0] = t.x; v[1] = t.y;
  } else {
#pragma unroll
    for (int s = 0; s < STRIDE; s += 4) {
      const float4 t = reinterpret_cast<const float4*>(p)[(size_t)g * (STRIDE / 4) + s / 4];
      v[s] = t.x; v[s + 1] = t.y; v[s + 2] = t.z; v[s + 3] = t.w;
    }
  }
}

}  // namespace rg

#define RG_REQUIRE(cond, code, ...)  \
  do {                               \
    if (!(cond)) {                   \
      rg::set_error(__VA_ARGS__);    \
      return (code);                 \
    }                                \
  } while (0)
