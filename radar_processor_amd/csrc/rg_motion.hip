// Echo motion and nowcasts (include/radargrid_hip.h, rg_block_match_u8 / rg_advect_f32): planes quantised to 8-bit levels,
// one motion vector per block by exhaustive normalised cross-correlation, and the semi-Lagrangian extrapolation of a plane.
//
// The block match is the one stage here with arithmetic density: B*B multiply-adds per candidate, (2R+1)^2 candidates per
// block.  One workgroup owns one block: it stages the block and its (B+2R)^2 search window in LDS as packed bytes, then
// every thread takes candidates (dy, dx) in turn and forms Sab, Sb and Sbb with the packed 8-bit dot product
// (v_dot4_u32_u8), four pixels per instruction.  A window row at byte offset dx + R is read as aligned LDS dwords and
// byte-aligned in registers (v_alignbyte_b32); the block's dword is the same address in every lane (an LDS broadcast).
// The inner loop is integer only; each candidate ends in one float64 division and square root, and its score stays in LDS
// for the arg-max over the full tie key and for the parabola.  Integer sums do not depend on their order, the float64
// steps are rounded once each: every output is bit-reproducible.
#include <limits.h>
#include <math.h>
#include <string.h>

#include "rg_common.hpp"
#include "rg_motion_field.hpp"
#include "rg_sample.hpp"

namespace {

constexpr int kWaves = rg::kBlock / rg::kWave;
constexpr uint32_t kOnes = 0x01010101u;
constexpr int kKeyShift = 13;                    // tie key = (dy*dy + dx*dx) << 13 | candidate index (< 65^2 < 2^13)
enum { kNearest = 0, kBilinear = 1 };

// ---- quantise ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(rg::kBlock) void quantize_kernel(const float* __restrict__ src, const uint8_t* __restrict__ mask,
                                                              long n, float lo, float inv_step, uint8_t* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = src[i];
  uint8_t q = 0;
  if (!(mask && mask[i]) && v >= lo) {
    const float t = (v - lo) * inv_step;
    q = (uint8_t)(1 + (t >= 254.0f ? 254 : (int)t));
  }
  out[i] = q;
}

// ---- block match ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t dot4(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_udot4(a, b, c, false); }

__device__ __forceinline__ int nonzero_bytes(uint32_t d) {
  return ((d & 0xFFu) != 0) + ((d & 0xFF00u) != 0) + ((d & 0xFF0000u) != 0) + ((d & 0xFF000000u) != 0);
}

// sum of v over the workgroup, returned to every thread; `slots` holds kWaves words
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* slots) {
#pragma unroll
  for (int o = rg::kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o);
  __syncthreads();                               // the slots' previous readers are done
  if ((threadIdx.x & (rg::kWave - 1)) == 0) slots[threadIdx.x / rg::kWave] = v;
  __syncthreads();
  uint32_t total = 0;
#pragma unroll
  for (int k = 0; k < kWaves; ++k) total += slots[k];
  return total;
}

// (s, key) beats (s2, key2): the larger score, then the smaller tie key
__device__ __forceinline__ bool beats(double s, int key, double s2, int key2) { return s > s2 || (s == s2 && key < key2); }

__device__ __forceinline__ double parabola(const double* scores, int c, int step, bool has_m, bool has_p, double s0) {
  if (!(has_m && has_p)) return 0.0;
  const double m = scores[c - step], p = scores[c + step];
  if (isnan(m) || isnan(p)) return 0.0;          // an unqualified neighbour
  const double den = m - 2.0 * s0 + p;
  if (!(den < 0.0)) return 0.0;
  const double off = 0.5 * (m - p) / den;
  return off < -0.5 ? -0.5 : (off > 0.5 ? 0.5 : off);
}

// dynamic LDS: double scores[(2R+1)^2] | uint32 block[B * B/4] | uint32 window[(B+2R) * pitch], pitch = (B+2R)/4 + 2 dwords
__host__ __device__ inline int window_pitch(int B, int R) { return (B + 2 * R) / 4 + 2; }

__global__ __launch_bounds__(rg::kBlock) void block_match_kernel(const uint8_t* __restrict__ prev,
                                                                 const uint8_t* __restrict__ next, int h, int w, int B, int S,
                                                                 int R, int min_echo, int nby, int nbx,
                                                                 int16_t* __restrict__ disp, float* __restrict__ motion,
                                                                 float* __restrict__ score) {
  extern __shared__ __align__(8) unsigned char lds[];
  __shared__ uint32_t slots[kWaves];
  __shared__ double best_s[kWaves];
  __shared__ int best_key[kWaves];
  const int side = 2 * R + 1, n_cand = side * side;
  const int bdw = B / 4, W = B + 2 * R, pitch = window_pitch(B, R);
  double* scores = reinterpret_cast<double*>(lds);
  uint32_t* blk = reinterpret_cast<uint32_t*>(scores + n_cand);
  uint32_t* win = blk + B * bdw;

  const long id = blockIdx.x;                    // ((pair * nby) + by) * nbx + bx: the row of every output
  const long per_plane = (long)nby * nbx;
  const long pair = id / per_plane;
  const int by = (int)((id - pair * per_plane) / nbx), bx = (int)(id - pair * per_plane - (long)by * nbx);
  const int y0 = by * S, x0 = bx * S;
  const uint8_t* pp = prev + (size_t)pair * h * w;
  const uint8_t* np = next + (size_t)pair * h * w;

  // the block: wholly inside the plane; rows are not dword aligned, so bytes are loaded and packed
  uint32_t sa = 0, saa = 0, echo = 0;
  for (int i = threadIdx.x; i < B * bdw; i += rg::kBlock) {
    const int r = i / bdw, k = i - r * bdw;
    const uint8_t* p = pp + (size_t)(y0 + r) * w + (x0 + 4 * k);
    const uint32_t d = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    blk[i] = d;
    sa = dot4(d, kOnes, sa);
    saa = dot4(d, d, saa);
    echo += nonzero_bytes(d);
  }
  // the window: rows y0 - R .. y0 + B + R - 1, columns x0 - R ..; a byte outside the plane (or beyond the window) is 0
  for (int i = threadIdx.x; i < W * pitch; i += rg::kBlock) {
    const int r = i / pitch, k = i - r * pitch;
    const int y = y0 - R + r;
    uint32_t d = 0;
    if (y >= 0 && y < h) {
      const uint8_t* row = np + (size_t)y * w;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int cw = 4 * k + j, x = x0 - R + cw;
        if (cw < W && x >= 0 && x < w) d |= (uint32_t)row[x] << (8 * j);
      }
    }
    win[i] = d;
  }
  sa = block_sum(sa, slots);
  saa = block_sum(saa, slots);
  echo = block_sum(echo, slots);                 // its barriers also publish blk and win
  const long N = (long)B * B;
  const long va = N * (long)saa - (long)sa * (long)sa;
  if ((int)echo < min_echo || va <= 0) {         // uniform over the workgroup
    if (threadIdx.x == 0) {
      disp[2 * id] = 0;
      disp[2 * id + 1] = 0;
      motion[2 * id] = motion[2 * id + 1] = score[id] = __builtin_nanf("");
    }
    return;
  }

  double my_s = -2.0;                            // below every score
  int my_key = INT_MAX;
  for (int c = threadIdx.x; c < n_cand; c += rg::kBlock) {
    const int cy = c / side, cx = c - cy * side; // dy + R, dx + R: the window's row and byte column of this candidate
    const int dy = cy - R, dx = cx - R;
    double s = __builtin_nan("");
    if (y0 + dy >= 0 && y0 + dy + B <= h && x0 + dx >= 0 && x0 + dx + B <= w) {
      const uint32_t shift = (uint32_t)cx & 3u;
      const uint32_t* wrow = win + cy * pitch + (cx >> 2);
      const uint32_t* brow = blk;
      uint32_t sab = 0, sb = 0, sbb = 0;
      for (int r = 0; r < B; ++r, wrow += pitch, brow += bdw) {
        uint32_t lo = wrow[0];
        for (int k = 0; k < bdw; ++k) {
          const uint32_t hi = wrow[k + 1];
          const uint32_t b = __builtin_amdgcn_alignbyte(hi, lo, shift);
          sab = dot4(brow[k], b, sab);
          sb = dot4(b, kOnes, sb);
          sbb = dot4(b, b, sbb);
          lo = hi;
        }
      }
      const long vb = N * (long)sbb - (long)sb * (long)sb;
      if (vb > 0) {
        const long num = N * (long)sab - (long)sa * (long)sb;
        s = (double)num / sqrt((double)va * (double)vb);
        const int key = ((dy * dy + dx * dx) << kKeyShift) | c;
        if (beats(s, key, my_s, my_key)) {
          my_s = s;
          my_key = key;
        }
      }
    }
    scores[c] = s;
  }
#pragma unroll
  for (int o = rg::kWave / 2; o > 0; o >>= 1) {
    const double s2 = __shfl_down(my_s, o);
    const int key2 = __shfl_down(my_key, o);
    if (beats(s2, key2, my_s, my_key)) {
      my_s = s2;
      my_key = key2;
    }
  }
  if ((threadIdx.x & (rg::kWave - 1)) == 0) {
    best_s[threadIdx.x / rg::kWave] = my_s;
    best_key[threadIdx.x / rg::kWave] = my_key;
  }
  __syncthreads();                               // ... and every score is in LDS
  if (threadIdx.x != 0) return;
  for (int k = 1; k < kWaves; ++k)
    if (beats(best_s[k], best_key[k], my_s, my_key)) {
      my_s = best_s[k];
      my_key = best_key[k];
    }
  if (my_key == INT_MAX) {                       // no qualified candidate
    disp[2 * id] = 0;
    disp[2 * id + 1] = 0;
    motion[2 * id] = motion[2 * id + 1] = score[id] = __builtin_nanf("");
    return;
  }
  const int c = my_key & ((1 << kKeyShift) - 1);
  const int cy = c / side, cx = c - cy * side;
  const double off_y = parabola(scores, c, side, cy > 0, cy < side - 1, my_s);
  const double off_x = parabola(scores, c, 1, cx > 0, cx < side - 1, my_s);
  disp[2 * id] = (int16_t)(cy - R);
  disp[2 * id + 1] = (int16_t)(cx - R);
  motion[2 * id] = (float)((double)(cy - R) + off_y);
  motion[2 * id + 1] = (float)((double)(cx - R) + off_x);
  score[id] = (float)my_s;
}

// ---- advect -----------------------------------------------------------------------------------------------------------------
struct Leads {
  double v[RG_MAX_LEADS];
};

// one thread per pixel and lead (blockIdx.y); src / out as bits where the value is only copied
template <int METHOD>
__global__ __launch_bounds__(rg::kBlock) void advect_kernel(const uint32_t* __restrict__ src, int n_planes, int h, int w,
                                                            const float* __restrict__ motion, rg_motion_lattice L, Leads leads,
                                                            int substeps, uint32_t fill, uint32_t* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t plane = (size_t)h * w;
  if (i >= (long)plane) return;
  const int y = (int)(i / w), x = (int)(i - (long)y * w);
  const double py = (double)y, px = (double)x;
  double v0y, v0x, dy, dx;
  rg::motion_at(motion, L, py, px, &v0y, &v0x);
  rg::displacement(motion, L, py, px, v0y, v0x, leads.v[blockIdx.y] / (double)substeps, substeps, &dy, &dx);
  const double fy = py - dy, fx = px - dx;
  uint32_t* o = out + (size_t)blockIdx.y * n_planes * plane + i;
  if constexpr (METHOD == kBilinear) {
    const rg::BilinearTaps taps = rg::bilinear_taps(fx, fy, w, h, true);
    for (int p = 0; p < n_planes; ++p) o[p * plane] = rg::bilinear_sample(src + p * plane, w, taps, fill);
  } else {
    size_t at;
    const bool inside = rg::nearest_node(fx, fy, w, h, true, &at);
    for (int p = 0; p < n_planes; ++p) o[p * plane] = inside ? src[p * plane + at] : fill;
  }
}

// the refusals every entry point here shares; *total = n * h * w
int check_planes(const char* who, int32_t n, int32_t h, int32_t w, int64_t* total) {
  RG_REQUIRE(n >= 1, RG_EINVAL, "%s: the number of planes must be at least 1", who);
  RG_REQUIRE(h >= 0 && w >= 0, RG_EINVAL, "%s: negative size", who);
  *total = (int64_t)n * h * w;
  RG_REQUIRE(*total < (int64_t)1 << 31, RG_EINVAL, "%s: n * h * w must stay below 2^31", who);
  return RG_OK;
}

}  // namespace

extern "C" int rg_motion_quantize_f32(const float* src, const uint8_t* mask, int32_t n, int32_t h, int32_t w, float lo,
                                      float inv_step, uint8_t* out, rg_stream_t stream) {
  const char* who = "rg_motion_quantize_f32";
  RG_REQUIRE(src && out, RG_EINVAL, "%s: null pointer", who);
  int64_t total;
  const int status = check_planes(who, n, h, w, &total);
  if (status != RG_OK) return status;
  RG_REQUIRE(isfinite(lo) && isfinite(inv_step), RG_EINVAL, "%s: lo and inv_step must be finite", who);
  RG_REQUIRE(inv_step > 0.0f, RG_EINVAL, "%s: inv_step must be positive", who);
  if (total == 0) return RG_OK;
  hipLaunchKernelGGL(quantize_kernel, dim3((unsigned)((total + rg::kBlock - 1) / rg::kBlock)), dim3(rg::kBlock), 0,
                     (hipStream_t)stream, src, mask, (long)total, lo, inv_step, out);
  return rg::check_launch(who);
}

extern "C" int rg_block_match_u8(const uint8_t* prev, const uint8_t* next, int32_t n, int32_t h, int32_t w, int32_t block,
                                 int32_t stride, int32_t search, int32_t min_echo, int16_t* disp, float* motion, float* score,
                                 rg_stream_t stream) {
  const char* who = "rg_block_match_u8";
  RG_REQUIRE(prev && next && disp && motion && score, RG_EINVAL, "%s: null pointer", who);
  int64_t total;
  const int status = check_planes(who, n, h, w, &total);
  if (status != RG_OK) return status;
  RG_REQUIRE(block >= 4 && block <= RG_MOTION_MAX_BLOCK && block % 4 == 0, RG_EINVAL,
             "%s: block must be a multiple of 4 in 4 .. %d", who, RG_MOTION_MAX_BLOCK);
  RG_REQUIRE(stride >= 1, RG_EINVAL, "%s: stride must be at least 1", who);
  RG_REQUIRE(search >= 0 && search <= RG_MOTION_MAX_SEARCH, RG_EINVAL, "%s: search must lie in 0 .. %d", who,
             RG_MOTION_MAX_SEARCH);
  RG_REQUIRE(min_echo >= 1 && min_echo <= block * block, RG_EINVAL, "%s: min_echo must lie in 1 .. block * block", who);
  RG_REQUIRE(h >= block && w >= block, RG_EINVAL, "%s: the planes are smaller than a block", who);
  const int nby = (h - block) / stride + 1, nbx = (w - block) / stride + 1;
  const int side = 2 * search + 1;
  const size_t lds = (size_t)side * side * sizeof(double) +
                     ((size_t)block * (block / 4) + (size_t)(block + 2 * search) * window_pitch(block, search)) * 4;
  hipLaunchKernelGGL(block_match_kernel, dim3((unsigned)((int64_t)n * nby * nbx)), dim3(rg::kBlock), lds, (hipStream_t)stream,
                     prev, next, h, w, block, stride, search, min_echo, nby, nbx, disp, motion, score);
  return rg::check_launch(who);
}

extern "C" int rg_advect_f32(const float* src, int32_t n_planes, int32_t h, int32_t w, const float* motion,
                             rg_motion_lattice lattice, const double* leads_host, int32_t n_leads, int32_t substeps,
                             int32_t method, float fill, float* out, rg_stream_t stream) {
  const char* who = "rg_advect_f32";
  RG_REQUIRE(src && motion && out && (leads_host || n_leads == 0), RG_EINVAL, "%s: null pointer", who);
  int64_t total;
  const int status = check_planes(who, n_planes, h, w, &total);
  if (status != RG_OK) return status;
  RG_REQUIRE(n_leads >= 0 && n_leads <= RG_MAX_LEADS, RG_EINVAL, "%s: n_leads must lie in 0 .. %d", who, RG_MAX_LEADS);
  Leads leads = {};
  for (int l = 0; l < n_leads; ++l) {
    RG_REQUIRE(isfinite(leads_host[l]), RG_EINVAL, "%s: lead %d is not finite", who, l);
    leads.v[l] = leads_host[l];
  }
  RG_REQUIRE(isfinite(lattice.origin_y) && isfinite(lattice.origin_x) && isfinite(lattice.step_y) && isfinite(lattice.step_x),
             RG_EINVAL, "%s: a member of rg_motion_lattice is not finite", who);
  RG_REQUIRE(lattice.step_y > 0.0 && lattice.step_x > 0.0, RG_EINVAL, "%s: step_y and step_x must be positive", who);
  RG_REQUIRE(lattice.ny >= 1 && lattice.nx >= 1, RG_EINVAL, "%s: ny and nx must be at least 1", who);
  RG_REQUIRE(substeps >= 1 && substeps <= 16, RG_EINVAL, "%s: substeps must lie in 1 .. 16", who);
  RG_REQUIRE(method == kNearest || method == kBilinear, RG_EINVAL, "%s: unknown method %d", who, method);
  RG_REQUIRE(!rg::overlap(src, total * 4, out, total * 4 * n_leads), RG_EINVAL, "%s: out overlaps src", who);
  if (total == 0 || n_leads == 0) return RG_OK;
  uint32_t fill_bits;
  memcpy(&fill_bits, &fill, sizeof fill_bits);
  const dim3 grid((unsigned)(((int64_t)h * w + rg::kBlock - 1) / rg::kBlock), (unsigned)n_leads);
  if (method == kNearest)
    hipLaunchKernelGGL(advect_kernel<kNearest>, grid, dim3(rg::kBlock), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint32_t*>(src), n_planes, h, w, motion, lattice, leads, substeps, fill_bits,
                       reinterpret_cast<uint32_t*>(out));
  else
    hipLaunchKernelGGL(advect_kernel<kBilinear>, grid, dim3(rg::kBlock), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint32_t*>(src), n_planes, h, w, motion, lattice, leads, substeps, fill_bits,
                       reinterpret_cast<uint32_t*>(out));
  return rg::check_launch(who);
}
