// The motion field of include/radargrid_hip.h ("motion at a point", "displacement"): the bilinear interpolant of a node
// lattice and the backward semi-Lagrangian displacement built from it.  Shared by the advection (rg_motion.hip) and the
// advection-corrected accumulation (rg_accumulate.hip), so that both reach the same float64 source position for the same
// pixel and lead, bit for bit.  Built with FP contraction off like every unit: the steps are the header's, in its order.
#pragma once

#include <math.h>

#include "rg_common.hpp"

namespace rg {

__device__ __forceinline__ double clamp_node(double l, int n) {        // NaN -> 0: no index is ever formed from a NaN
  const double hi = (double)(n - 1);
  return !(l >= 0.0) ? 0.0 : (l > hi ? hi : l);
}

// the header's "motion at a point": both components of the lattice's bilinear interpolant, constant beyond its rim
__device__ __forceinline__ void motion_at(const float* __restrict__ motion, const rg_motion_lattice& L, double py, double px,
                                          double* vy, double* vx) {
  const double ly = clamp_node((py - L.origin_y) / L.step_y, L.ny), lx = clamp_node((px - L.origin_x) / L.step_x, L.nx);
  const int j0 = min((int)floor(ly), max(L.ny - 2, 0)), i0 = min((int)floor(lx), max(L.nx - 2, 0));
  const int j1 = min(j0 + 1, L.ny - 1), i1 = min(i0 + 1, L.nx - 1);
  const double ty = ly - (double)j0, tx = lx - (double)i0;
  const float* v00 = motion + 2 * ((size_t)j0 * L.nx + i0), *v01 = motion + 2 * ((size_t)j0 * L.nx + i1);
  const float* v10 = motion + 2 * ((size_t)j1 * L.nx + i0), *v11 = motion + 2 * ((size_t)j1 * L.nx + i1);
  *vy = ((double)v00[0] * (1.0 - tx) + (double)v01[0] * tx) * (1.0 - ty) + ((double)v10[0] * (1.0 - tx) + (double)v11[0] * tx) * ty;
  *vx = ((double)v00[1] * (1.0 - tx) + (double)v01[1] * tx) * (1.0 - ty) + ((double)v10[1] * (1.0 - tx) + (double)v11[1] * tx) * ty;
}

// the header's "displacement" of pixel (py, px) after `lead` intervals: d = (0, 0); `substeps` times d = d + dt * V(p - d) with
// dt = lead / (double)substeps, which the caller forms (it is the same for every pixel).  The first step reads
// V(p - 0) = V(p), which does not depend on the lead: the caller evaluates it once per pixel (motion_at at (py, px)) and passes
// it as (v0y, v0x), so a kernel that needs several leads of one pixel pays for it once -- with substeps == 1 no other lattice
// read remains.
__device__ __forceinline__ void displacement(const float* __restrict__ motion, const rg_motion_lattice& L, double py, double px,
                                             double v0y, double v0x, double dt, int substeps, double* dy_out, double* dx_out) {
  double dy = 0.0 + dt * v0y, dx = 0.0 + dt * v0x;
  for (int k = 1; k < substeps; ++k) {
    double vy, vx;
    motion_at(motion, L, py - dy, px - dx, &vy, &vx);
    dy = dy + dt * vy;
    dx = dx + dt * vx;
  }
  *dy_out = dy;
  *dx_out = dx;
}

}  // namespace rg
