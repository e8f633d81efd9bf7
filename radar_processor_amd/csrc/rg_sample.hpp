// The two rules by which a float32 plane [ny][nx] is sampled at a float64 position (fx, fy) in nodes
// (include/radargrid_hip.h, rg_warp_mercator_f32): shared by the Web Mercator warp (rg_warp.hip) and the advection
// (rg_motion.hip), so that both give the same bits for the same position.  Planes are moved as their bits where a value
// is only copied.  Built with FP contraction off like every unit: the steps are the header's, in its order.
#pragma once

#include <math.h>

#include "rg_common.hpp"

namespace rg {

// nearest: the node floor(f + 0.5) per axis; false (and *at = 0) where it lies outside the plane or the position is not usable
__device__ __forceinline__ bool nearest_node(double fx, double fy, int nx, int ny, bool usable, size_t* at) {
  const double gx = floor(fx + 0.5), gy = floor(fy + 0.5);
  const bool inside = usable && gx >= 0.0 && gx < (double)nx && gy >= 0.0 && gy < (double)ny;
  *at = inside ? (size_t)gy * nx + (size_t)gx : 0;
  return inside;
}

// bilinear: the four taps (y0,x0), (y0,x0+1), (y0+1,x0), (y0+1,x0+1) and their float64 weights, set up once per position
struct BilinearTaps {
  double w[4];
  int x0, y0;
  bool in_x[2], in_y[2];
  bool near;                     // false: no tap is inside the plane (or the position is not usable)
};

__device__ __forceinline__ BilinearTaps bilinear_taps(double fx, double fy, int nx, int ny, bool usable) {
  BilinearTaps t;
  t.near = usable && fx > -1.0 && fx < (double)nx && fy > -1.0 && fy < (double)ny;
  const double x0f = floor(fx), y0f = floor(fy);
  const double tx = fx - x0f, ty = fy - y0f;
  t.x0 = t.near ? (int)x0f : 0;
  t.y0 = t.near ? (int)y0f : 0;
  t.w[0] = (1.0 - ty) * (1.0 - tx);
  t.w[1] = (1.0 - ty) * tx;
  t.w[2] = ty * (1.0 - tx);
  t.w[3] = ty * tx;
  t.in_x[0] = t.x0 >= 0;
  t.in_x[1] = t.x0 + 1 < nx;
  t.in_y[0] = t.y0 >= 0;
  t.in_y[1] = t.y0 + 1 < ny;
  return t;
}

// one plane through the taps: a tap outside the plane, or a NaN one, is missing; the value while the present weights sum
// to at least 0.5, else `fill`
__device__ __forceinline__ uint32_t bilinear_sample(const uint32_t* __restrict__ plane, int nx, const BilinearTaps& t,
                                                    uint32_t fill) {
  double wsum = 0.0, vsum = 0.0;
  if (t.near) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!(t.in_y[k >> 1] && t.in_x[k & 1])) continue;
      const float v = bits_f32(plane[(size_t)(t.y0 + (k >> 1)) * nx + (t.x0 + (k & 1))]);
      if (isnan(v)) continue;
      wsum += t.w[k];
      vsum += t.w[k] * (double)v;
    }
  }
  return wsum >= 0.5 ? f32_bits((float)(vsum / wsum)) : fill;
}

}  // namespace rg
