// Shared pieces of the ROI neighbour search: the geometry builder, the fused lattice / mosaic gridder (rg_roi_grid.hip) and
// the section gridder (rg_roi_section.hip) all stream the same cell-sorted gate lists, and every rule they have in common
// is written here ONCE -- the radius of influence and its rim band, the membership test, what happens to a hit, the
// candidate stream.  The two kernels keep what differs for measured reasons (their header comments): the lane layout, the
// pre-filter, the value ring, the closest-gate mode, the radar visits.
//
// Include only from translation units compiled with -ffp-contract=off: the float64 expressions below are the reference's
// unfused NumPy arithmetic and must stay unfused; the float32 tests use explicit fmaf, whose error the rim band covers.
#pragma once

#include <type_traits>

#include "rg_common.hpp"

namespace rg {
namespace roi {

struct Cells {
  double x0, y0, inv_cx, inv_cy, z_lo, z_hi;
  int ncx, ncy;
  int levels;      // > 1: per-level gate lists, the cells of level iz at iz * ncx * ncy
  int level0;      // ... and the level the call's zc[0] is
};

inline Cells to_cells(const rg_cellgrid* c) {
  Cells r;
  r.x0 = c->x0; r.y0 = c->y0; r.inv_cx = c->inv_cx; r.inv_cy = c->inv_cy; r.z_lo = c->z_lo; r.z_hi = c->z_hi;
  r.ncx = c->ncx; r.ncy = c->ncy;
  r.levels = c->levels > 1 ? c->levels : 0;
  r.level0 = c->levels > 1 ? c->level0 : 0;
  return r;
}

__device__ __forceinline__ double cell_coord(double g, double origin, double inv) { return floor((g - origin) * inv); }

__device__ __forceinline__ int cell_clamped(double g, double origin, double inv, int n) {
  const double t = cell_coord(g, origin, inv);
  return t < 0.0 ? 0 : (t >= (double)n ? n - 1 : (int)t);
}

struct SearchArgs {
  const rg_gate4* sorted;
  const int* cell_start;
  Cells c;
  const float* xc;
  const float* yc;
  const float* zc;
  int nz, ny, nx;
  long n_vox;
  double min_radius, beam_factor;
};

// A vertical section (rg_roi_section.hip): n_points sample columns at arbitrary (xs[i], ys[i]) times the nz levels of zc.
// The search structure is the lattice's own: its cell lists and bounds do not depend on where the samples lie, as long as
// they lie inside the rectangle the structure was built for.
struct SectionArgs {
  const rg_gate4* sorted;
  const int* cell_start;
  Cells c;
  const float* xs;
  const float* ys;
  const float* zc;
  int nz, n_points;
  long n_samples;      // nz * n_points
  double min_radius, beam_factor;
};

template <int W>
__device__ __forceinline__ float roi_weight(double d2, double r2) {
  if constexpr (W == RG_W_BARNES2) {
    return (float)(exp(-d2 / (r2 / 4.0)) + 1e-5);  // compute.py:83
  } else if constexpr (W == RG_W_CRESSMAN) {
    return (float)((r2 - d2) / (r2 + d2));         // compute.py:85
  } else {
    return 1.0f;                                    // compute.py:87 ('nearest' = uniform mean)
  }
}

// What the dense stage does with a (record, sample) hit:
//   kGridMode   accumulate the masked weighted mean (rg_roi_grid_f32, rg_roi_grid_mosaic_f32, rg_roi_section_f32)
//   kCountMode  count it                            (rg_geom_count_f32, rg_section_count_f32: row lengths of the CSR)
//   kFillMode   append (gate index, float64-exact weight) to the sample's CSR row (rg_geom_fill_f32, rg_section_fill_f32)
// Count and fill classify hits with the same code, so the second pass writes exactly what the first one counted; a
// sample's hits arrive in (cell row, sorted position) order, the row order the CSR has always had.
constexpr int kGridMode = 0, kCountMode = 1, kFillMode = 2;

__device__ __forceinline__ double readlane_f64(double v, int lane) {
  const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)b, lane);
  const unsigned hi = __builtin_amdgcn_readlane((unsigned)(b >> 32), lane);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ float readlane_f32(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// release / barrier / acquire around every hand-over between the candidate stage (which writes the wave's LDS ring) and the
// dense stage (which reads it with another lane assignment), and back before drained slots are written again
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- the rim band -------------------------------------------------------------------------------------------------------
// The float32 d2 of in_roi() carries < 4e-7 relative error, so outside [r2 * (1 - 2e-6), r2 * (1 + 2e-6)] the float32
// comparison already decides as the float64 one would; the second factor (1 +- 2.4e-7 = 2 ulp) covers the rounding of the
// bound itself to float32.  These two numbers are the only place the band is written: the candidate pre-filters of both
// kernels inflate the block's largest radius with band_hi, and the per-voxel error bound every grid is tested against
// (oracle.mean_error_bound, tests/test_gpu_mean_bounds.py) is a statement about them.
__device__ __forceinline__ float band_hi(double r2) { return (float)(r2 * (1.0 + 2e-6)) * (1.0f + 2.4e-7f); }
__device__ __forceinline__ float band_lo(double r2) { return (float)(r2 * (1.0 - 2e-6)) * (1.0f - 2.4e-7f); }

// One sample (a voxel of the lattice, a point of a section at one level): the reference's float64 radius of influence
// (compute.py:46-47,57) and its float32 bounds.  A lane that is not live (outside the grid, outside a radar's window, a
// non-finite point) gets the empty band (-1, -1): it never hits.
struct Sample {
  double x, y, z, r, r2;
  float xf, yf, zf, r2f;
  float r2_lo, r2_hi;      // band_lo / band_hi of r2
  float inv_r2q;           // Barnes: MINUS log2(e) * 4 / r2, see weight_from_f32
};

__device__ __forceinline__ Sample make_sample(double x, double y, double z, bool live, double min_radius, double beam_factor) {
  Sample s;
  s.x = x; s.y = y; s.z = z;
  const double dist = sqrt(x * x + y * y + z * z);
  s.r = fmax(min_radius, dist * beam_factor);
  s.r2 = s.r * s.r;
  s.xf = (float)x; s.yf = (float)y; s.zf = (float)z;     // grid coordinates ARE float32 values: exact
  s.r2f = (float)s.r2;
  s.r2_hi = live ? band_hi(s.r2) : -1.0f;
  s.r2_lo = live ? band_lo(s.r2) : -1.0f;                // dead lanes never hit
  s.inv_r2q = (float)(-1.4426950408889634 * 4.0 / s.r2);
  return s;
}

// The largest radius of influence among the N samples of a block (N consecutive lanes, a power of two; wave-uniform result)
template <int N>
__device__ __forceinline__ double block_max_radius(const Sample& s, bool live) {
  double rmax = live ? s.r : 0.0;
#pragma unroll
  for (int m = 1; m < N; m <<= 1) rmax = fmax(rmax, __shfl_xor(rmax, m, 64));
  return readlane_f64(rmax, 0);
}

// The membership rule.  float32 d2 decides whenever it is clear of the rim by the band; inside the band the reference's
// exact float64 `d2 < r2` (compute.py:69-74) decides, so the neighbour set equals the CSR builder's.  `valid`: the lane
// holds a record at all (a caller that has established that passes true and the tests fold away).  d2f is set either way.
__device__ __forceinline__ bool in_roi(const rg_gate4& g, const Sample& s, bool valid, float& d2f) {
  const float dx = g.x - s.xf, dy = g.y - s.yf, dz = g.z - s.zf;
  d2f = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
  bool in = valid && d2f <= s.r2_lo;
  if (valid && !in && d2f <= s.r2_hi) {  // within 2e-6 of the rim: the reference's float64 arithmetic decides
    const double ex = (double)g.x - s.x, ey = (double)g.y - s.y, ez = (double)g.z - s.z;  // compute.py:69-71
    in = ex * ex + ey * ey + ez * ez < s.r2;                                              // compute.py:72,74
  }
  return in;
}

// The reference's float64 d2 of a (record, sample) pair (compute.py:69-72), unfused
__device__ __forceinline__ double d2_f64(const rg_gate4& g, const Sample& s) {
  const double ex = (double)g.x - s.x, ey = (double)g.y - s.y, ez = (double)g.z - s.z;
  return ex * ex + ey * ey + ez * ez;
}

// Builder modes, one dense step: count this step's hits of the lane's sample and (fill) append them to its CSR row.
// Executed by every lane of the wave (__ballot).  own_lanes: the lanes that test records against the same sample as this
// one (one per record slot); lower_slots: those of them with a lower slot -- their hits come first in the row.  cursor:
// hits of the sample so far, identical in all of its lanes.  The weight is the float64-exact one, rounded once.
template <int MODE, int W>
__device__ __forceinline__ void emit_hit(bool in, const rg_gate4& g, const Sample& s, unsigned long long own_lanes,
                                         unsigned long long lower_slots, long long row_base, int& cursor,
                                         int* __restrict__ gidx, float* __restrict__ wts) {
  const unsigned long long hits = __ballot(in);
  if constexpr (MODE == kFillMode) {
    if (in) {
      const double d2 = d2_f64(g, s);                                                 // compute.py:72
      const long long pos = row_base + cursor + __popcll(hits & lower_slots);
      gidx[pos] = g.index;
      wts[pos] = roi_weight<W>(d2, s.r2);                                             // compute.py:82-87
    }
  }
  cursor += __popcll(hits & own_lanes);
}

// float32 weight from the float32 d2 (compute.py:82-87): Barnes (>= e^-4 inside the ROI) and uniform; relative error
// < 2e-6 (d2f and inv_r2q carry a few u each; 2^x turns the exponent's absolute error, up to 5.8 * 6u, into a relative
// one of ln 2 times that).  Not Cressman, whose numerator r2 - d2 cancels near the rim (grid_weight takes it from the
// float64 d2).  inv_r2q: Barnes -- MINUS log2(e) * 4 / r2, so that exp(-d2 / (r2 / 4)) is one multiply and one v_exp_f32 (= 2^x)
template <int W>
__device__ __forceinline__ float weight_from_f32(float d2f, float inv_r2q) {
  static_assert(W != RG_W_CRESSMAN, "Cressman's numerator comes from the float64 d2 (grid_weight)");
  if constexpr (W == RG_W_BARNES2) {
    return __builtin_amdgcn_exp2f(d2f * inv_r2q) + 1e-5f;
  } else {
    return 1.0f;
  }
}

// Grid mode: the weight of a hit.  Barnes and uniform in float32 (Barnes |rel err| < 2e-6 against compute.py's float64
// weight, uniform exact).  Cressman (r2 - d2) / (r2 + d2), compute.py:85: the numerator cancels at the rim -- from the
// float32 d2 it can be 0 or negative for a gate the float64 test admitted.  Numerator from the reference's float64 d2
// (unfused, as the test: r2 - d2 > 0 for every hit), rounded once; denominator in float32 (no cancellation): |rel err| < 5e-7.
// These budgets are the delta of the per-voxel error bound (oracle.mean_error_bound) every grid of these kernels is tested
// against, and are observed directly by tests/test_gpu_mean_bounds.py's two-gate probes (worst measured: Barnes 5.1e-7,
// Cressman 1.6e-7, uniform 0).
template <int W>
__device__ __forceinline__ float grid_weight(const rg_gate4& g, const Sample& s, float d2f) {
  if constexpr (W == RG_W_CRESSMAN) {
    return (float)(s.r2 - d2_f64(g, s)) / (s.r2f + d2f);                              // compute.py:72,85
  } else {
    return weight_from_f32<W>(d2f, s.inv_r2q);
  }
}

// Grid mode, weighted modes: add a hit's packed field slots into the lane's sums (acc_p = sum w*v, acc_w = sum w); a slot
// that holds the exclusion pattern (rg_pack_fields_f32 folded the masks in) adds nothing.
template <int NF, int STRIDE>
__device__ __forceinline__ void accumulate(float w, const float (&val)[STRIDE], float (&acc_p)[NF], float (&acc_w)[NF]) {
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const bool ok = rg::f32_bits(val[f]) != RG_EXCLUDED_BITS;
    acc_p[f] += ok ? w * val[f] : 0.0f;  // float32 product, as interpolate.py:82
    acc_w[f] += ok ? w : 0.0f;
  }
}

// ---- how a mosaic combines its radars (rg_combine, radargrid_hip.h) ------------------------------------------------------
// RG_COMBINE_MEAN adds every radar's hits into one set of sums (the kernels' own visit loops; nothing here is used).  Under
// RG_COMBINE_MAX / RG_COMBINE_NEAREST_RADAR every radar of the table finishes its OWN mean at the end of its visit -- sums
// from zero, the final fold's shuffles, the final store's division: the bits the mean entry point stores for a table
// holding that radar alone -- and offers it to the sample's held value.  The winner's bits are copied, never computed with.

// D of a sample seen from the radar being visited: the float64, unfused expression make_sample forms under its sqrt
__device__ __forceinline__ double antenna_d2(double x, double y, double z) { return x * x + y * y + z * z; }

// The take-over test, the one place it is written.  has: radar k has a value (its live weight sum is > 0); any: a value is
// held already.  The table is walked in order, so staying on equality gives ties to the earlier position: equal values and
// -0.0 against +0.0 under MAX (neither is > the other), equal D under NEAREST_RADAR.  MAX: a held NaN yields to a number.
template <int COMBINE>
__device__ __forceinline__ bool takes_over(bool has, float m, double d, bool any, float held, double held_d) {
  static_assert(COMBINE == RG_COMBINE_MAX || COMBINE == RG_COMBINE_NEAREST_RADAR, "the mean holds nothing");
  if constexpr (COMBINE == RG_COMBINE_MAX) {
    return has && (!any || m > held || (held != held && m == m));
  } else {
    return has && (!any || d < held_d);
  }
}

// A sample's held state for NF fields (the choice is per field: masks are): the value, under NEAREST_RADAR the holder's D,
// and the holder's table position, eight bits a field packed four to a register (255: nothing held).  Identical in all
// lanes that own the sample.  The mean keeps none.
template <int COMBINE, int NF>
struct Held {
  float v[NF];
  double d[COMBINE == RG_COMBINE_NEAREST_RADAR ? NF : 1];
  unsigned who[(NF + 3) / 4];

  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int f = 0; f < NF; ++f) v[f] = 0.0f;
#pragma unroll
    for (int f = 0; f < (COMBINE == RG_COMBINE_NEAREST_RADAR ? NF : 1); ++f) d[f] = 0.0;
#pragma unroll
    for (int q = 0; q < (NF + 3) / 4; ++q) who[q] = 0xFFFFFFFFu;
  }
  __device__ __forceinline__ unsigned radar(int f) const { return (who[f >> 2] >> (8 * (f & 3))) & 0xFFu; }
  __device__ __forceinline__ void offer(int f, int k, bool has, float m, double dk) {
    constexpr bool NEAREST = COMBINE == RG_COMBINE_NEAREST_RADAR;
    const bool take = takes_over<COMBINE>(has, m, dk, radar(f) != 0xFFu, v[f], d[NEAREST ? f : 0]);
    v[f] = take ? m : v[f];
    if constexpr (NEAREST) d[f] = take ? dk : d[f];
    const unsigned sh = 8u * (unsigned)(f & 3);
    who[f >> 2] = take ? (who[f >> 2] & ~(0xFFu << sh)) | ((unsigned)k << sh) : who[f >> 2];
  }
};
template <int NF>
struct Held<RG_COMBINE_MEAN, NF> {};

// The end of radar k's visit under MAX / NEAREST_RADAR: fold the record slots of every field exactly as the mean's final
// fold does (xor shuffles over FIRST, 2 * FIRST, .. 32 -- the lanes that own one sample; each ends with the same bits), form
// the radar's ratio as the mean's final store does, offer it, and clear the sums for the next radar.  dk: antenna_d2.
template <int COMBINE, int FIRST, int NF>
__device__ __forceinline__ void finish_visit(int k, double dk, float (&acc_p)[NF], float (&acc_w)[NF], Held<COMBINE, NF>& held) {
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    float p = acc_p[f], w = acc_w[f];
#pragma unroll
    for (int m = FIRST; m < 64; m <<= 1) { p += __shfl_xor(p, m, 64); w += __shfl_xor(w, m, 64); }
    held.offer(f, k, w > 0.0f, (float)((double)p / (double)w), dk);
    acc_p[f] = 0.0f; acc_w[f] = 0.0f;
  }
}

// ---- the candidate stream -------------------------------------------------------------------------------------------------
// The cells a block's search box covers: its xy box widened by its largest radius (all wave-uniform)
struct CellBox {
  int cx0, cx1, cy0, cy1;
};

__device__ __forceinline__ CellBox cell_box(float xlo, float xhi, float ylo, float yhi, double rmax, const Cells& c) {
  CellBox b;
  b.cx0 = __builtin_amdgcn_readfirstlane(cell_clamped((double)xlo - rmax, c.x0, c.inv_cx, c.ncx));
  b.cx1 = __builtin_amdgcn_readfirstlane(cell_clamped((double)xhi + rmax, c.x0, c.inv_cx, c.ncx));
  b.cy0 = __builtin_amdgcn_readfirstlane(cell_clamped((double)ylo - rmax, c.y0, c.inv_cy, c.ncy));
  b.cy1 = __builtin_amdgcn_readfirstlane(cell_clamped((double)yhi + rmax, c.y0, c.inv_cy, c.ncy));
  return b;
}

// Up to 64 cell rows of the box and the walk over their candidates, 64 per step.  The chain cell_start -> gate record that
// would make the search latency-bound is broken here: the bounds of all rows come with one vector load each (lane <-> cell
// row) and are handed out with readlane; all walking state is wave-uniform.
struct CellRows {
  int rs_l, re_l;          // this lane's cell row: first and one-past-last sorted position
  int nr, row, jb, je;     // rows held; the current row and the current step's range [jb, je) in it

  __device__ __forceinline__ CellRows(const int* cell_start, int lvl_off, int ncx, const CellBox& b, int rb, int nrows,
                                      int lane) {
    rs_l = 0; re_l = 0;
    if (rb + lane < nrows) {
      const int base = lvl_off + (b.cy0 + rb + lane) * ncx;
      rs_l = cell_start[base + b.cx0];
      re_l = cell_start[base + b.cx1 + 1];
    }
    nr = nrows - rb < 64 ? nrows - rb : 64;
    row = -1; jb = 0; je = 0;
  }

  __device__ __forceinline__ bool advance() {  // next 64-candidate step
    jb += 64;
    while (jb >= je) {
      if (++row >= nr) return false;
      jb = __builtin_amdgcn_readlane(rs_l, row);
      je = __builtin_amdgcn_readlane(re_l, row);
    }
    return true;
  }
};

// Survivors of a candidate step are compacted into the wave's ring: this lane's position (meaningful where it survived),
// m = __ballot(survived); the caller advances tail by __popcll(m).
__device__ __forceinline__ int ring_position(unsigned long long m, int tail) {
  return tail + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// The candidate loop itself (bounds, advance, prefetch, pre-filter, append, drain when 64 wait) stays written out in both
// kernels.  As one function taking the pre-filter and the queue / drain steps as callables it compiled to about 20 more
// scalar instructions per value-ring kernel and cost six lattice instantiations a wave of occupancy.  The lattice kernel
// also keeps its own bounds load and advance() lambda: with CellRows two of its instantiations lose a wave and two mosaic
// ones spill two more SGPRs (profiles/roi_core_resource_usage.txt).

// ---- host side ------------------------------------------------------------------------------------------------------------
inline int check_search_args(const char* fn, const rg_gate4* sorted, const int32_t* cell_start, const rg_cellgrid* cells,
                             const float* xc, const float* yc, const float* zc, int nz, int ny, int nx) {
  RG_REQUIRE(sorted && cell_start && cells && xc && yc && zc, RG_EINVAL, "%s: null pointer", fn);
  RG_REQUIRE(nz >= 1 && ny >= 1 && nx >= 1, RG_EINVAL, "%s: bad grid shape (%d,%d,%d)", fn, nz, ny, nx);
  RG_REQUIRE(cells->ncx >= 1 && cells->ncy >= 1 && (long)cells->ncx * cells->ncy < 0x7FFFFFFFL, RG_EINVAL,
             "%s: bad cell grid %dx%d", fn, cells->ncx, cells->ncy);
  RG_REQUIRE(rg::aligned16(sorted), RG_EALIGN, "%s: sorted_gates must be 16-byte aligned", fn);
  RG_REQUIRE(cells->levels <= 1 || (cells->level0 >= 0 && cells->level0 + nz <= cells->levels &&
                                    (long)cells->ncx * cells->ncy * cells->levels < 0x7FFFFFFFL), RG_EINVAL,
             "%s: per-level gate lists for %d levels, call covers levels %d .. %d (or too many cells)", fn, cells->levels,
             cells->level0, cells->level0 + nz - 1);
  return RG_OK;
}

// Weighting of a builder (fill) or gridding entry point: RG_W_BARNES2 .. w_max.  no_closest: why the closest-gate mode is
// refused as unsupported rather than as unknown (nullptr: no such distinction).
inline int check_weighting(const char* fn, int weighting, int w_max, const char* no_closest) {
  if (no_closest) RG_REQUIRE(weighting != RG_W_CLOSEST, RG_EUNSUPPORTED, "%s: the closest-gate mode is %s", fn, no_closest);
  RG_REQUIRE(weighting >= RG_W_BARNES2 && weighting <= w_max, RG_EINVAL, "%s: unknown weighting %d", fn, weighting);
  return RG_OK;
}

// What the three gridding entry points (lattice, mosaic, section) ask of their weighting and field arguments
inline int check_grid_args(const char* fn, const float* packed, const float* out, int weighting, int w_max,
                           const char* no_closest, int n_fields, int stride) {
  RG_REQUIRE(packed && out, RG_EINVAL, "%s: null pointer", fn);
  const int rc = check_weighting(fn, weighting, w_max, no_closest);
  if (rc != RG_OK) return rc;
  RG_REQUIRE(n_fields >= 1 && n_fields <= RG_MAX_FIELDS, RG_EUNSUPPORTED, "%s: n_fields=%d not in 1..%d", fn, n_fields,
             RG_MAX_FIELDS);
  RG_REQUIRE(stride == rg::stride_for(n_fields), RG_EINVAL, "%s: stride=%d, expected %d for %d fields", fn, stride,
             rg::stride_for(n_fields), n_fields);
  RG_REQUIRE(rg::aligned16(packed), RG_EALIGN, "%s: packed must be 16-byte aligned", fn);
  return RG_OK;
}

// The combine rule of a mosaic entry point (rg_combine) and its provenance output, which the joint mean does not have
inline int check_combine(const char* fn, int combine, const void* out_radar) {
  RG_REQUIRE(combine >= RG_COMBINE_MEAN && combine <= RG_COMBINE_NEAREST_RADAR, RG_EINVAL, "%s: unknown combine rule %d", fn,
             combine);
  RG_REQUIRE(combine != RG_COMBINE_MEAN || out_radar == nullptr, RG_EINVAL,
             "%s: out_radar with RG_COMBINE_MEAN (a joint mean has no one radar behind it)", fn);
  return RG_OK;
}

inline SearchArgs make_args(const rg_gate4* sorted, const int32_t* cell_start, const rg_cellgrid* cells, const float* xc,
                            const float* yc, const float* zc, int nz, int ny, int nx, double min_radius,
                            double beam_factor) {
  SearchArgs a;
  a.sorted = sorted; a.cell_start = cell_start; a.c = to_cells(cells);
  a.xc = xc; a.yc = yc; a.zc = zc; a.nz = nz; a.ny = ny; a.nx = nx;
  a.n_vox = (long)nz * ny * nx;
  a.min_radius = min_radius; a.beam_factor = beam_factor;
  return a;
}

// weighting (checked by the caller) -> f(int_c<W>); the closest-gate mode only where the entry point has one
template <bool WITH_CLOSEST = false, class F>
int dispatch_weighting(int weighting, F&& f) {
  if constexpr (WITH_CLOSEST) {
    if (weighting == RG_W_CLOSEST) return f(int_c<RG_W_CLOSEST>{});
  }
  switch (weighting) {
    case RG_W_BARNES2: return f(int_c<RG_W_BARNES2>{});
    case RG_W_CRESSMAN: return f(int_c<RG_W_CRESSMAN>{});
    default: return f(int_c<RG_W_NEAREST>{});
  }
}

// combine (RG_COMBINE_MAX or RG_COMBINE_NEAREST_RADAR, checked by the caller; the mean has its own launch) -> f(int_c<COMBINE>)
template <class F>
int dispatch_combine(int combine, F&& f) {
  return combine == RG_COMBINE_MAX ? f(int_c<RG_COMBINE_MAX>{}) : f(int_c<RG_COMBINE_NEAREST_RADAR>{});
}

}  // namespace roi
}  // namespace rg
