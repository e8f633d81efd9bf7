// The footprint sum shared by the disk background and the convective area (include/radargrid_hip.h, "Convective / stratiform
// classification"): a footprint is a table of half-widths per row distance, a table row holds the EXCLUSIVE prefix of a
// quantity along x with w + 1 entries (entry 0 is zero, entry x + 1 the sum over columns 0 .. x), and the sum over a footprint
// is one difference of two entries per covered row.  Entries are integers, so the differences are exact whatever the order.
#pragma once

#include "rg_common.hpp"

namespace rg {

// passed to the kernels BY VALUE; ry and the row distance are wave-uniform, so the half-widths are read through scalar loads:
// four to a 32-bit word, because the scalar unit loads no single bytes
struct Footprint {
  int32_t ry;
  uint32_t packed[(RG_MAX_DISK_RADIUS + 1) / 4];
  __host__ __device__ int hw(int d) const { return (int)((packed[d >> 2] >> ((d & 3) * 8)) & 255u); }
};

// 0 .. ry <= RG_MAX_DISK_RADIUS and every half-width in 0 .. RG_MAX_DISK_RADIUS; fills `out`
inline int read_footprint(const char* who, const int32_t* hw_host, int32_t ry, Footprint* out) {
  RG_REQUIRE(ry >= 0 && ry <= RG_MAX_DISK_RADIUS, RG_EINVAL, "%s: ry must lie in 0 .. %d, got %d", who, RG_MAX_DISK_RADIUS, ry);
  *out = Footprint{};
  out->ry = ry;
  for (int d = 0; d <= ry; ++d) {
    RG_REQUIRE(hw_host[d] >= 0 && hw_host[d] <= RG_MAX_DISK_RADIUS, RG_EINVAL, "%s: hw[%d] must lie in 0 .. %d, got %d", who, d,
               RG_MAX_DISK_RADIUS, hw_host[d]);
    out->packed[d >> 2] |= (uint32_t)hw_host[d] << ((d & 3) * 8);
  }
  return RG_OK;
}

// entries per table row
__host__ __device__ inline size_t prefix_pitch(int w) { return (size_t)w + 1; }

// The sum over the footprint at (y, x) of one plane's prefix table, the footprint cut to the plane.  `y` must be wave-uniform
// (the callers give one row to a wavefront), 0 <= y < h and 0 <= x < w.  Entry::Sum has `add(hi, lo)`, which accumulates
// hi - lo.  Rows max(y - ry, 0) .. min(y + ry, h - 1) -- at most 255 trips; columns max(x - hw, 0) .. min(x + hw, w - 1),
// i.e. entries max(x - hw, 0) and min(x + hw, w - 1) + 1, both in 0 .. w: every index is formed from clamped coordinates.
// UNROLL rows' loads are issued together.
template <int UNROLL, class Entry>
__device__ __forceinline__ typename Entry::Sum disk_sum(const Entry* __restrict__ table, int h, int w, int y, int x,
                                                        const Footprint& fp) {
  typename Entry::Sum sum{};
  const int r0 = max(y - fp.ry, 0), r1 = min(y + fp.ry, h - 1);
  const size_t pitch = prefix_pitch(w);
#pragma unroll UNROLL
  for (int r = r0; r <= r1; ++r) {
    const int half = fp.hw(abs(r - y));
    const Entry* row = table + (size_t)r * pitch;
    sum.add(row[min(x + half, w - 1) + 1], row[max(x - half, 0)]);
  }
  return sum;
}

// a count per entry: the per-class centre tables of the convective area
struct CountEntry {
  int32_t c;
  struct Sum {
    int32_t c;
    __device__ __forceinline__ void add(const CountEntry& hi, const CountEntry& lo) { c += hi.c - lo.c; }
  };
};

}  // namespace rg
