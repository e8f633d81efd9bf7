// Vertical cross-section along any path, straight from the gates: K2's arithmetic (rg_roi_grid.hip --
// radar_grid/compute.py:46-91 fused with radar_grid/interpolate.py:69-104) evaluated at sample columns (xs[i], ys[i]) that
// need not form a lattice.  Sample (k, i) -- level k, point i -- is what the reference would put into a voxel lying exactly
// at (xs[i], ys[i], zc[k]); row k * n_points + i is the row order of a grid of shape (nz, 1, n_points).
//
// Structure (one wavefront = kPts = 4 consecutive points of one level, lanes = 4 points x 16 record slots):
//   * the candidate cells come from the bounding box of the block's own points -- wave reductions over the lanes' x and y,
//     no coordinate table has ends to read -- widened by the block's largest radius of influence.  Nothing assumes that
//     consecutive points are close: a block of scattered points has a large box and streams many candidates, and still
//     finds exactly its neighbours;
//   * candidate stage (lanes = 64 candidates per step): the float32 distance to the nearest of four sub-boxes of kPts / 4
//     points each -- with 4 points per block, to the nearest POINT -- against band_hi of the block's largest radius.  With
//     one point per sub-box this is in_roi's float32 d2 with the squares added in another order, so it is no lower bound
//     to the last bit: the band's 2e-6 (five times the error of either sum) is what keeps every gate the dense stage
//     would admit.  A path runs at any angle through the cells, so the block's box is mostly far from it; the sub-boxes
//     follow it;
//   * dense stage: K2's, 16 queued records per step, through the same functions of rg_roi_search.hpp (in_roi: float32 d2
//     where it is clear of the rim band, the reference's float64 `d2 < r2` inside it; grid_weight / accumulate: float32
//     weights within K2's budgets; emit_hit: count and fill classify hits with the same code, fill writes the float64-exact
//     weight rounded to float32).  Grid mode gathers the packed field slots per hit; a point's hits arrive in (cell row,
//     sorted position) order, the row order the CSR has always had;
//   * the survivor ring holds at most 63 waiting + 64 new records and is drained whenever 64 are waiting, so a row of
//     thousands of neighbours (a section through the radar) passes through it like any other; row lengths and ring
//     positions are 32-bit counts of gates, of which the search structure holds fewer than 2^31.
//
// Why 4 x 16 and not K2's 16 x 4: a section is a few thousand wavefronts, and where it passes the radar ONE block holds the
// rows of thousands of neighbours: the kernel's time is that block's wavefront (the time below does not depend on the number
// of points, only on whether the path passes the radar).  Measured on the bench volume, 2000 points x 40 levels along the diagonal of the 40 x 2000 x 2000 grid's rectangle: 16 x 4
// 1.65 ms through the radar (the same for 500 points) and 0.041 ms for a diagonal that misses it by 42 km; 4 x 16 0.30 ms
// and 0.035 ms (four times fewer dense steps for the heavy rows, four times as many wavefronts, a prefilter that is exact
// per point).  The lattice pass over the same structure (rg_roi_grid_f32) takes 10.9 ms.
//
// A point with a non-finite coordinate -- NaN, +Inf or -Inf in x, in y or in both -- has no neighbours (its samples are
// filled, its rows counted as 0 and never written): the cell of a NaN is not defined, and with beam_factor > 0 an infinite
// coordinate alone would make the radius of influence infinite and every candidate a neighbour, so BOTH coordinates are
// tested.  Such a point is a dead lane: it adds nothing to the block's radius, sub-boxes or cell box, and a block of dead
// points only streams no cells at all.  Points outside the rectangle the search structure was built for read clamped cells:
// memory-safe, but their neighbours are not guaranteed -- the Python surface refuses both before a launch.
// (tests/test_gpu_section_rim.py calls the C entry points with dead points in every mix per block.)
//
// Several radars on one section (rg_roi_section_mosaic_f32, MOSAIC): the block visits the radars of the table in order.  For
// each it rebuilds its samples from that radar's own xs / ys / zc (the points in that radar's frame: the distance to the
// antenna, hence the radius of influence, differs per radar), its sub-boxes and cell box from that radar's cells, streams
// that radar's candidates, gathers from that radar's part of the packed fields and adds the hits into the ONE set of float32
// accumulators; the ring is drained before the next radar starts, so a radar's candidates never move another radar's slot
// assignment -- one radar at gate offset 0 gives the bits of rg_roi_section_f32.  A point a radar cannot serve carries a NaN
// in that radar's arrays (dead, as above); a block without a live point skips the radar before anything of its search
// structure is read, and an entry without gates is skipped before its points are.  The table travels by value in the kernel
// arguments (16 x 112 bytes) and is indexed with the wave-uniform visit number: scalar loads, no scratch.
// With a combine rule (rg_roi_section_mosaic_combine_f32, COMBINE = RG_COMBINE_MAX / RG_COMBINE_NEAREST_RADAR) every radar's
// visit ends with rg_roi_search.hpp's finish_visit -- the radar's own mean of each sample and field, offered to the held
// value, the sums cleared -- and the final store writes what is held; RG_COMBINE_MEAN compiles none of it.
//
// Compiled with -ffp-contract=off like every TU (the exact test must not be fused); the float32 tests use explicit fmaf,
// their error is covered by the rim band (rg_roi_search.hpp).
#include "rg_common.hpp"
#include "rg_roi_search.hpp"

namespace {

using namespace rg::roi;
using rg::dispatch_fields;

constexpr int kRing = 128;   // survivor queue per wave (power of two): <= 63 waiting + 64 new records
constexpr int kPts = 4;      // points per block
constexpr int kLgPts = 2;
constexpr int kSlots = 64 / kPts;   // queued records tested per dense step
static_assert(1 << kLgPts == kPts && kPts >= 4 && kPts <= 16, "lane = slot * kPts + point; four sub-boxes of kPts / 4 points");

constexpr unsigned long long slot_lanes_of_point0() {   // the lanes that own point 0: one per record slot
  unsigned long long m = 0;
  for (int s = 0; s < kSlots; ++s) m |= 1ull << (s * kPts);
  return m;
}

// One radar of a mosaic section: its search structure, the points and levels in its frame, its gate 0 inside the shared
// packed fields.  sorted == nullptr: the radar takes no part (no gates, or no search structure) and nothing of it is read.
struct SectionRadar {
  const rg_gate4* sorted;
  const int* cell_start;
  Cells c;
  const float* xs;
  const float* ys;
  const float* zc;
  const float* packed;
};
struct SectionMosaicArgs {
  SectionRadar r[RG_MAX_RADARS];
  int n_radars;
  int nz, n_points;
  long n_samples;      // nz * n_points
  double min_radius, beam_factor;
  unsigned char* out_radar;   // RG_COMBINE_MAX / _NEAREST_RADAR: who supplied the value (or null)
};

template <int MODE, int W, int NF, int STRIDE, bool MOSAIC = false, int COMBINE = RG_COMBINE_MEAN>
__global__ __launch_bounds__(rg::kBlock) void section_kernel(std::conditional_t<MOSAIC, SectionMosaicArgs, SectionArgs> a,
                                                             const float* __restrict__ packed, float fill,
                                                             float* __restrict__ out, int* __restrict__ counts,
                                                             const long long* __restrict__ indptr, int* __restrict__ gidx,
                                                             float* __restrict__ wts) {
  static_assert(!MOSAIC || MODE == kGridMode, "the mosaic section grids; its CSR is built radar by radar");
  static_assert(MOSAIC || COMBINE == RG_COMBINE_MEAN, "one radar has nothing to combine");
  __shared__ rg_gate4 ring_all[rg::kBlock / rg::kWave][kRing];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  rg_gate4* ring = ring_all[wv];
  // 32-bit on purpose (a 64-bit division is a few hundred instructions); the launcher guarantees that the count fits
  const unsigned bpl = ((unsigned)a.n_points + (unsigned)(kPts - 1)) / (unsigned)kPts;   // blocks per level
  const unsigned wave = blockIdx.x * (unsigned)(rg::kBlock / rg::kWave) + (unsigned)wv;
  const unsigned iz_l = wave / bpl;
  if (iz_l >= (unsigned)a.nz) return;                                           // wave-uniform
  const int iz = (int)iz_l;
  const int i0 = (int)(wave - iz_l * bpl) * kPts;
  const int pl = lane & (kPts - 1);                                             // point of the block this lane owns
  const int slot = lane >> kLgPts;                                              // which of the kSlots records of a dense step
  const int ip = i0 + pl;
  const bool inside = ip < a.n_points;

  // acc_p = sum w*v, acc_w = sum w (this lane's point, this lane's record slot; with MOSAIC over all radars)
  float acc_p[NF], acc_w[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) { acc_p[f] = 0.0f; acc_w[f] = 0.0f; }
  Held<COMBINE, NF> held;    // MAX / NEAREST_RADAR: per field the winner so far (the mean: empty)
  if constexpr (COMBINE != RG_COMBINE_MEAN) held.clear();
  int head = 0, tail = 0;    // ring positions (wave-uniform, monotone; head == tail between two radars)
  // builder modes: hits of this lane's point so far (identical in the point's slot lanes) and its row base
  int cursor = 0;
  long long row_base = 0;
  const size_t row = (size_t)iz * (size_t)a.n_points + (size_t)(inside ? ip : 0);
  if constexpr (MODE == kFillMode) {
    if (inside) row_base = indptr[row];
  }
  const unsigned long long pt_lanes = slot_lanes_of_point0() << pl;             // the slot lanes of point pl
  const unsigned long long lower_slots = pt_lanes & ((1ull << (kPts * slot)) - 1ull);

  int n_visits = 1;
  if constexpr (MOSAIC) n_visits = a.n_radars;
  for (int visit = 0; visit < n_visits; ++visit) {
  // the search structure, the points and the levels of the radar being visited (the only one without MOSAIC)
  const rg_gate4* sorted;
  const int* cell_start;
  const float *pxs, *pys, *pzc, *pk;
  if constexpr (MOSAIC) {
    const SectionRadar& R = a.r[visit];
    if (R.sorted == nullptr) continue;                                          // takes no part (wave-uniform): nothing is read
    sorted = R.sorted; cell_start = R.cell_start; pxs = R.xs; pys = R.ys; pzc = R.zc; pk = R.packed;
  } else {
    sorted = a.sorted; cell_start = a.cell_start; pxs = a.xs; pys = a.ys; pzc = a.zc; pk = packed;
  }
  // ---- this lane's sample: the reference's float64 ROI (compute.py:46-47,57) and its float32 bounds ----------------
  const float xf = inside ? pxs[ip] : 0.0f, yf = inside ? pys[ip] : 0.0f;
  const bool live = inside && __builtin_isfinite(xf) && __builtin_isfinite(yf);
  if constexpr (MOSAIC) {
    if (__ballot(live) == 0ull) continue;                                       // no point of the block is the radar's (wave-uniform)
  }
  Cells c;
  if constexpr (MOSAIC) c = a.r[visit].c; else c = a.c;
  const int lvl_off = c.levels > 1 ? (c.level0 + iz) * (c.ncx * c.ncy) : 0;     // per-level gate lists: this level's cells
  const double z = (double)pzc[iz];                                             // common to the whole wave
  const float zf = (float)z;
  const Sample s = make_sample(live ? (double)xf : 0.0, live ? (double)yf : 0.0, z, live, a.min_radius, a.beam_factor);
  // ---- block-wide (wave-uniform) quantities: largest radius, the four sub-boxes and the block's box ----------------
  const double rmax = block_max_radius<kPts>(s, live);
  const float inf = __builtin_inff();
  float bxlo = live ? xf : inf, bxhi = live ? xf : -inf, bylo = live ? yf : inf, byhi = live ? yf : -inf;
#pragma unroll
  for (int m = 1; m < kPts / 4; m <<= 1) {                                      // the lane's sub-box: kPts / 4 consecutive points
    bxlo = fminf(bxlo, __shfl_xor(bxlo, m, 64)); bxhi = fmaxf(bxhi, __shfl_xor(bxhi, m, 64));
    bylo = fminf(bylo, __shfl_xor(bylo, m, 64)); byhi = fmaxf(byhi, __shfl_xor(byhi, m, 64));
  }
  float sxlo[4], sxhi[4], sylo[4], syhi[4];                                     // an empty sub-box is (+inf, -inf): nothing is near it
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    sxlo[k] = readlane_f32(bxlo, kPts / 4 * k); sxhi[k] = readlane_f32(bxhi, kPts / 4 * k);
    sylo[k] = readlane_f32(bylo, kPts / 4 * k); syhi[k] = readlane_f32(byhi, kPts / 4 * k);
  }
  const float xlo = fminf(fminf(sxlo[0], sxlo[1]), fminf(sxlo[2], sxlo[3]));
  const float xhi = fmaxf(fmaxf(sxhi[0], sxhi[1]), fmaxf(sxhi[2], sxhi[3]));
  const float ylo = fminf(fminf(sylo[0], sylo[1]), fminf(sylo[2], sylo[3]));
  const float yhi = fmaxf(fmaxf(syhi[0], syhi[1]), fmaxf(syhi[2], syhi[3]));
  const bool any_live = xlo <= xhi;                                             // wave-uniform
  const float r2max_hi = band_hi(rmax * rmax);
  CellBox box = {0, -1, 0, -1};
  if (any_live) box = cell_box(xlo, xhi, ylo, yhi, rmax, c);

  auto dense = [&](int n) {  // test n queued records against the block's points, kSlots records per step
    for (int e0 = 0; e0 < n; e0 += kSlots) {
      const int e = e0 + slot;
      bool in = false;
      rg_gate4 g;
      g.x = g.y = g.z = 0.0f; g.index = 0;
      float d2f = 0.0f;
      if (e < n) {
        g = ring[(head + e) & (kRing - 1)];
        in = in_roi(g, s, true, d2f);
      }
      if constexpr (MODE != kGridMode) {
        emit_hit<MODE, W>(in, g, s, pt_lanes, lower_slots, row_base, cursor, gidx, wts);
      } else if (in) {
        float val[STRIDE];
        rg::load_packed<STRIDE>(pk, (unsigned)g.index, val);                              // one gather per hit
        accumulate<NF>(grid_weight<W>(g, s, d2f), val, acc_p, acc_w);
      }
    }
    head += n;
  };

  const int nrows = box.cy1 - box.cy0 + 1;
  for (int rb = 0; rb < nrows; rb += 64) {
    CellRows rows(cell_start, lvl_off, c.ncx, box, rb, nrows, lane);
    bool have = rows.advance();
    rg_gate4 gn;
    gn.x = gn.y = gn.z = 0.0f; gn.index = 0;
    bool vn = false;
    if (have) { vn = rows.jb + lane < rows.je; if (vn) gn = sorted[rows.jb + lane]; }
    while (have) {
      const rg_gate4 g = gn;
      const bool valid = vn;
      have = rows.advance();
      if (have) { vn = rows.jb + lane < rows.je; if (vn) gn = sorted[rows.jb + lane]; }  // prefetch the next step
      // lower bound of the distance to the nearest sub-box vs the block's largest (inflated) radius
      const float dz = g.z - zf;
      const float dz2 = dz * dz;
      bool pre = false;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float dxb = fmaxf(fmaxf(sxlo[k] - g.x, g.x - sxhi[k]), 0.0f);
        const float dyb = fmaxf(fmaxf(sylo[k] - g.y, g.y - syhi[k]), 0.0f);
        pre = pre || __builtin_fmaf(dxb, dxb, __builtin_fmaf(dyb, dyb, dz2)) <= r2max_hi;
      }
      pre = pre && valid;
      const unsigned long long m = __ballot(pre);
      if (pre) ring[ring_position(m, tail) & (kRing - 1)] = g;
      tail += __popcll(m);
      if (tail - head >= 64) {
        wave_sync();
        dense(64);
        wave_sync();   // the drained slots are written again from here on
      }
    }
  }
  wave_sync();
  dense(tail - head);
  if constexpr (MOSAIC) wave_sync();   // the next radar writes the ring from here on
  if constexpr (COMBINE != RG_COMBINE_MEAN) {
    finish_visit<COMBINE, kPts>(visit, COMBINE == RG_COMBINE_NEAREST_RADAR ? antenna_d2(s.x, s.y, s.z) : 0.0, acc_p, acc_w, held);
  }
  }  // visit

  if constexpr (MODE == kCountMode) {
    if (slot == 0 && inside) counts[row] = cursor;
    return;
  } else if constexpr (MODE == kFillMode) {
    return;
  } else if constexpr (COMBINE != RG_COMBINE_MEAN) {
    if (slot == 0 && inside) {   // the slot lanes of a point hold the same bits
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const unsigned who = held.radar(f);
        out[(size_t)f * (size_t)a.n_samples + row] = who != 0xFFu ? held.v[f] : fill;
        if (a.out_radar) a.out_radar[(size_t)f * (size_t)a.n_samples + row] = (unsigned char)who;
      }
    }
  } else {
    // ---- fold the record slots; lanes 0 .. kPts - 1 hold the block's points, consecutive samples of the level -------
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      float p = acc_p[f], w = acc_w[f];
#pragma unroll
      for (int m = kPts; m < 64; m <<= 1) { p += __shfl_xor(p, m, 64); w += __shfl_xor(w, m, 64); }
      if (slot == 0 && inside) out[(size_t)f * (size_t)a.n_samples + row] = w > 0.0f ? (float)((double)p / (double)w) : fill;
    }
  }
}

inline long section_waves(int nz, int n_points) { return (((long)n_points + kPts - 1) / kPts) * nz; }

inline int check_section_args(const char* fn, const rg_gate4* sorted, const int32_t* cell_start, const rg_cellgrid* cells,
                              const float* xs, const float* ys, const float* zc, int nz, int n_points) {
  RG_REQUIRE(sorted && cell_start && cells && xs && ys && zc, RG_EINVAL, "%s: null pointer", fn);
  RG_REQUIRE(nz >= 1 && n_points >= 1, RG_EINVAL, "%s: bad section shape (nz=%d, n_points=%d)", fn, nz, n_points);
  const int rc = check_search_args(fn, sorted, cell_start, cells, xs, ys, zc, nz, 1, n_points);
  if (rc != RG_OK) return rc;
  RG_REQUIRE(section_waves(nz, n_points) < 0xFFFFFFF0L, RG_EUNSUPPORTED, "%s: section too large for one launch", fn);
  return RG_OK;
}

inline SectionArgs make_section_args(const rg_gate4* sorted, const int32_t* cell_start, const rg_cellgrid* cells,
                                     const float* xs, const float* ys, const float* zc, int nz, int n_points,
                                     double min_radius, double beam_factor) {
  SectionArgs a;
  a.sorted = sorted; a.cell_start = cell_start; a.c = to_cells(cells);
  a.xs = xs; a.ys = ys; a.zc = zc; a.nz = nz; a.n_points = n_points;
  a.n_samples = (long)nz * n_points;
  a.min_radius = min_radius; a.beam_factor = beam_factor;
  return a;
}

template <int MODE, int W, int NF, int STRIDE, bool MOSAIC = false, int COMBINE = RG_COMBINE_MEAN, class Args>
int launch(const char* fn, const Args& a, const float* packed, float fill, float* out, int* counts,
           const long long* indptr, int* gidx, float* wts, hipStream_t s) {
  hipLaunchKernelGGL((section_kernel<MODE, W, NF, STRIDE, MOSAIC, COMBINE>), dim3((unsigned)((section_waves(a.nz, a.n_points) + 3) / 4)),
                     dim3(rg::kBlock), 0, s, a, packed, fill, out, counts, indptr, gidx, wts);
  return rg::check_launch(fn);
}

}  // namespace

extern "C" int rg_roi_section_f32(const rg_gate4* sorted_gates, const int32_t* cell_start, const rg_cellgrid* cells_host,
                                  const float* xs, const float* ys, const float* zc, int32_t nz, int32_t n_points,
                                  double min_radius, double beam_factor, int32_t weighting, const float* packed,
                                  int32_t n_fields, int32_t stride, float fill_value, float* out, rg_stream_t stream) {
  const char* fn = "rg_roi_section_f32";
  int rc = check_grid_args(fn, packed, out, weighting, RG_W_NEAREST, "a lattice mode", n_fields, stride);
  if (rc != RG_OK) return rc;
  rc = check_section_args(fn, sorted_gates, cell_start, cells_host, xs, ys, zc, nz, n_points);
  if (rc != RG_OK) return rc;
  const SectionArgs a = make_section_args(sorted_gates, cell_start, cells_host, xs, ys, zc, nz, n_points, min_radius,
                                          beam_factor);
  return dispatch_weighting(weighting, [&](auto w) {
    return dispatch_fields(n_fields, [&](auto nf, auto st) {
      return launch<kGridMode, decltype(w)::value, decltype(nf)::value, decltype(st)::value>(
          fn, a, packed, fill_value, out, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream);
    });
  });
}

// A section through several radars: per radar, radar_grid/compute.py:46-91 at the points in that radar's frame, and
// radar_grid/interpolate.py:69-104 over the union of all radars' neighbours.  Every refusal happens before any launch.
namespace {
int section_mosaic(const char* fn, const rg_section_radar* radars_host, int32_t n_radars, int32_t nz, int32_t n_points,
                   double min_radius, double beam_factor, int32_t weighting, const float* packed, int32_t n_fields,
                   int32_t stride, int64_t n_gates_total, float fill_value, float* out, int32_t combine,
                   unsigned char* out_radar, rg_stream_t stream) {
  RG_REQUIRE(radars_host, RG_EINVAL, "%s: null radar table", fn);
  RG_REQUIRE(n_radars >= 1, RG_EINVAL, "%s: n_radars=%d", fn, n_radars);
  RG_REQUIRE(n_radars <= RG_MAX_RADARS, RG_EUNSUPPORTED, "%s: n_radars=%d exceeds %d", fn, n_radars, RG_MAX_RADARS);
  RG_REQUIRE(nz >= 1 && n_points >= 1, RG_EINVAL, "%s: bad section shape (nz=%d, n_points=%d)", fn, nz, n_points);
  int rc = check_grid_args(fn, packed, out, weighting, RG_W_NEAREST, "a single-radar lattice mode", n_fields, stride);
  if (rc != RG_OK) return rc;
  rc = check_combine(fn, combine, out_radar);
  if (rc != RG_OK) return rc;
  // the gather takes a 32-bit slot number (rg::load_packed)
  RG_REQUIRE(n_gates_total >= 0 && n_gates_total <= 0x7FFFFFFFL, RG_EUNSUPPORTED,
             "%s: n_gates_total=%lld not in 0 .. 2^31 - 1", fn, (long long)n_gates_total);
  RG_REQUIRE(section_waves(nz, n_points) < 0xFFFFFFF0L, RG_EUNSUPPORTED, "%s: section too large for one launch", fn);
  SectionMosaicArgs a = {};
  a.n_radars = n_radars;
  a.nz = nz; a.n_points = n_points;
  a.n_samples = (long)nz * n_points;
  a.min_radius = min_radius; a.beam_factor = beam_factor;
  a.out_radar = out_radar;
  for (int r = 0; r < n_radars; ++r) {
    const rg_section_radar& e = radars_host[r];
    // the kernel gathers packed[gate_offset + index] through a raw pointer: the offsets are what keep it in bounds
    RG_REQUIRE(e.gate_offset >= 0 && e.n_gates >= 0 && e.gate_offset + e.n_gates <= n_gates_total, RG_EINVAL,
               "%s: radar %d: gates %lld + %lld exceed n_gates_total=%lld", fn, r, (long long)e.gate_offset,
               (long long)e.n_gates, (long long)n_gates_total);
    if (e.n_gates == 0 || e.sorted_gates == nullptr) continue;   // takes no part: never visited, pointers not read
    rc = check_section_args(fn, e.sorted_gates, e.cell_start, &e.cells, e.xs, e.ys, e.zc, nz, n_points);
    if (rc != RG_OK) return rc;
    SectionRadar& m = a.r[r];
    m.sorted = e.sorted_gates; m.cell_start = e.cell_start; m.c = to_cells(&e.cells);
    m.xs = e.xs; m.ys = e.ys; m.zc = e.zc;
    m.packed = packed + e.gate_offset * stride;
  }
  if (combine == RG_COMBINE_MEAN) {
    return dispatch_weighting(weighting, [&](auto w) {
      return dispatch_fields(n_fields, [&](auto nf, auto st) {
        return launch<kGridMode, decltype(w)::value, decltype(nf)::value, decltype(st)::value, true>(
            fn, a, nullptr, fill_value, out, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream);
      });
    });
  }
  return dispatch_weighting(weighting, [&](auto w) {
    return dispatch_fields(n_fields, [&](auto nf, auto st) {
      return dispatch_combine(combine, [&](auto cb) {
        return launch<kGridMode, decltype(w)::value, decltype(nf)::value, decltype(st)::value, true, decltype(cb)::value>(
            fn, a, nullptr, fill_value, out, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream);
      });
    });
  });
}
}  // namespace

extern "C" int rg_roi_section_mosaic_f32(const rg_section_radar* radars_host, int32_t n_radars, int32_t nz,
                                         int32_t n_points, double min_radius, double beam_factor, int32_t weighting,
                                         const float* packed, int32_t n_fields, int32_t stride, int64_t n_gates_total,
                                         float fill_value, float* out, rg_stream_t stream) {
  return section_mosaic("rg_roi_section_mosaic_f32", radars_host, n_radars, nz, n_points, min_radius, beam_factor, weighting,
                        packed, n_fields, stride, n_gates_total, fill_value, out, RG_COMBINE_MEAN, nullptr, stream);
}

// ... with a combine rule (rg_combine): RG_COMBINE_MEAN launches the kernel above, the other two their own instantiations
extern "C" int rg_roi_section_mosaic_combine_f32(const rg_section_radar* radars_host, int32_t n_radars, int32_t nz,
                                                 int32_t n_points, double min_radius, double beam_factor, int32_t weighting,
                                                 const float* packed, int32_t n_fields, int32_t stride,
                                                 int64_t n_gates_total, float fill_value, float* out, int32_t combine,
                                                 uint8_t* out_radar, rg_stream_t stream) {
  return section_mosaic("rg_roi_section_mosaic_combine_f32", radars_host, n_radars, nz, n_points, min_radius, beam_factor,
                        weighting, packed, n_fields, stride, n_gates_total, fill_value, out, combine, out_radar, stream);
}

// count -> prefix sum (rg_scan_counts_i64) -> fill: a section as an ordinary CSR of nz * n_points rows
extern "C" int rg_section_count_f32(const rg_gate4* sorted_gates, const int32_t* cell_start, const rg_cellgrid* cells_host,
                                    const float* xs, const float* ys, const float* zc, int32_t nz, int32_t n_points,
                                    double min_radius, double beam_factor, int32_t* counts, rg_stream_t stream) {
  const char* fn = "rg_section_count_f32";
  RG_REQUIRE(counts, RG_EINVAL, "%s: null counts", fn);
  const int rc = check_section_args(fn, sorted_gates, cell_start, cells_host, xs, ys, zc, nz, n_points);
  if (rc != RG_OK) return rc;
  const SectionArgs a = make_section_args(sorted_gates, cell_start, cells_host, xs, ys, zc, nz, n_points, min_radius,
                                          beam_factor);
  return launch<kCountMode, RG_W_NEAREST, 1, 1>(fn, a, nullptr, 0.0f, nullptr, counts, nullptr, nullptr, nullptr,
                                                (hipStream_t)stream);
}

extern "C" int rg_section_fill_f32(const rg_gate4* sorted_gates, const int32_t* cell_start, const rg_cellgrid* cells_host,
                                   const float* xs, const float* ys, const float* zc, int32_t nz, int32_t n_points,
                                   double min_radius, double beam_factor, int32_t weighting, const int64_t* indptr,
                                   int32_t* gate_idx, float* weights, rg_stream_t stream) {
  const char* fn = "rg_section_fill_f32";
  RG_REQUIRE(indptr && gate_idx && weights, RG_EINVAL, "%s: null pointer", fn);
  int rc = check_weighting(fn, weighting, RG_W_NEAREST, "a lattice mode");
  if (rc != RG_OK) return rc;
  rc = check_section_args(fn, sorted_gates, cell_start, cells_host, xs, ys, zc, nz, n_points);
  if (rc != RG_OK) return rc;
  const SectionArgs a = make_section_args(sorted_gates, cell_start, cells_host, xs, ys, zc, nz, n_points, min_radius,
                                          beam_factor);
  return dispatch_weighting(weighting, [&](auto w) {
    return launch<kFillMode, decltype(w)::value, 1, 1>(fn, a, nullptr, 0.0f, nullptr, nullptr,
                                                       reinterpret_cast<const long long*>(indptr), gate_idx, weights,
                                                       (hipStream_t)stream);
  });
}
