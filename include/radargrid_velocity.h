/* radargrid_velocity.h -- Doppler velocity dealiasing by regions: the fourth header of libradargrid_hip.so.
 *
 * The entry points declared here are compiled into the SAME library as those of the other three headers (csrc/rg_velocity.hip)
 * and follow the conventions of radargrid_phase.h: device pointers unless a name ends in _host, the stream last, every argument
 * validated and RG_EINVAL returned before anything touches the device, rg_last_error() text beginning with the function's name,
 * no allocation, no host synchronisation and no memset node (workspaces are cleared by a kernel, so the calls can be captured
 * into a hipGraph).  They live in a header of their own, bound from the table `_native.VELOCITY_SIGNATURES`, so that the other
 * three headers and their tables stay byte-identical: rg_velocity_split_f32, rg_velocity_regions_i32,
 * rg_region_edges_workspace_bytes, rg_region_edges_f32 and rg_velocity_apply_folds_f32 were ADDED; no signature changed,
 * RG_VERSION stays 104.
 *
 * The algorithm is the region-based one (PyART's dealias_region_based), restated so that every number the decision rests on is
 * an integer and every output is bit-reproducible:
 *   1  split [-Vn, Vn] into bands                               rg_velocity_split_f32
 *   2  label the connected regions of each band                 rg_label_components_f32 / rg_component_stats_f32 (radargrid_hip.h)
 *   3  flatten the labels to one region id per gate             rg_velocity_regions_i32
 *   4  build the table of touching regions                      rg_region_edges_f32
 *   5  merge the regions greedily by the strongest edge         on the host (velocity.merge_regions): a small graph problem
 *   6  add each region's whole number of Nyquist intervals      rg_velocity_apply_folds_f32
 * (No reference counterpart in radar_grid; the tests pin the kernels to the NumPy restatement of exactly these formulas,
 * tests/velocity_oracle.py.  Parity with PyART is unpinned.)
 *
 * Common definitions:
 *   A volume is vel float32 [S][R][G]: S >= 1 sweeps of R >= 1 rays of G >= 0 gates, row-major, S * R * G < 2^31; the entry
 *   points that see the split stack also require S * n_bands * R * G < 2^31 (what the labeller takes).
 *   mask (optional, may be NULL) uint8 of the same shape: non-zero leaves the gate out.
 *   nyquist_host double [S]: one Nyquist velocity Vn per sweep, each finite with 0 < Vn <= RG_VELOCITY_MAX_NYQUIST.  It is read
 *   on the host during the call and travels in the launch arguments, RG_VELOCITY_SWEEPS_PER_LAUNCH sweeps per launch.
 *   n_bands = B in RG_VELOCITY_MIN_BANDS .. RG_VELOCITY_MAX_BANDS.
 *   A gate (or a value) is VALID when it is finite, |v| <= RG_VELOCITY_MAX_ABS and its mask is 0.
 *   band   = clamp(floor(((double)v + Vn) * B / (2.0 * Vn)), 0, B - 1), float64 in that order, clamped before the conversion
 *            to int; a value beyond +-Vn falls into an end band.
 *   q      = llrint(65536 * (double)v): the fixed-point value, exact, |q| <= 2^30.
 *   I_s    = llrint(65536 * 2.0 * Vn_s): the Nyquist interval of sweep s in the same fixed point (the host side uses it).
 *   Every MISSING float32 output is the quiet NaN 0x7FC00000.  Float arithmetic is unfused, in the order written.
 */
#ifndef RADARGRID_VELOCITY_H
#define RADARGRID_VELOCITY_H

#include "radargrid_hip.h" /* rg_stream_t, the status codes */

#ifdef __cplusplus
extern "C" {
#endif

#define RG_VELOCITY_MAX_ABS 16384          /* m/s: |v| beyond it is not a valid gate, so that 65536 * v fits 2^30 */
#define RG_VELOCITY_MAX_NYQUIST 8192       /* m/s */
#define RG_VELOCITY_MIN_BANDS 2
#define RG_VELOCITY_MAX_BANDS 8
#define RG_VELOCITY_SWEEPS_PER_LAUNCH 64   /* Nyquist velocities one launch carries in its arguments */

/* ---------------------------------------------------------------------------------------------------
 * 1  Split a volume into its velocity bands.
 *
 * split float32 [S][B][R][G]: plane (s, b) holds v where the gate is valid and its band is b, the quiet NaN elsewhere.  One
 * thread per gate writes its B planes; one launch per RG_VELOCITY_SWEEPS_PER_LAUNCH sweeps.
 * The caller then labels the stack with rg_label_components_f32 as S * B planes of [R][G] with lo = -FLT_MAX, hi = +inf,
 * connectivity = 4 and wrap_rows as wanted (one call; planes never connect), and takes `area` from rg_component_stats_f32.
 * RG_EINVAL before any launch: a null vel, nyquist_host or split; S < 1, R < 1, G < 0; S * B * R * G >= 2^31; n_bands out of
 * range; a Nyquist velocity out of range; split overlapping vel or mask.  G == 0 returns RG_OK without a launch. */
int rg_velocity_split_f32(const float* vel, const uint8_t* mask, int32_t S, int32_t R, int32_t G, const double* nyquist_host,
                          int32_t n_bands, float* split, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * 2  Flatten the labelling of the split stack into one region id per gate.
 *
 * labels int32 [S][B][R][G] and cell_ptr int32 [S * B + 1] are what rg_label_components_f32 wrote for the stack.
 *   regions[s][r][g] = cell_ptr[s * B + b] + labels[s][b][r][g]    for the lowest b whose label there is > 0 and at most the
 *                      cell count of its plane (cell_ptr[s * B + b + 1] - cell_ptr[s * B + b]); 0 when there is none.
 * Ids are global, 1-based and equal the cell-table row + 1: `area` of rg_component_stats_f32 is indexed by id - 1.
 * RG_EINVAL before any launch: a null pointer; the size limits; n_bands out of range; regions overlapping labels or cell_ptr.
 * G == 0 returns RG_OK without a launch. */
int rg_velocity_regions_i32(const int32_t* labels, const int32_t* cell_ptr, int32_t S, int32_t R, int32_t G, int32_t n_bands,
                            int32_t* regions, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * 3  The region adjacency table: for every pair of touching regions, the pixel pairs they share and the exact sum of the value
 *    differences across their border.  Generic: any values and any region ids.
 *
 * values float32 and regions int32, both [n_planes][h][w], n_planes >= 1, h, w >= 0, n_planes * h * w < 2^31.
 * The FORWARD neighbours of pixel (y, x): (y, x + 1) when x + 1 < w; (y + 1, x) when y + 1 < h; and, with wrap_rows != 0 and
 * h >= 3, (0, x) for y = h - 1.  With h <= 2 the wrap adds nothing, so no pixel pair is counted twice.  Planes never pair.
 * A pixel and a forward neighbour with regions a != b, both > 0, and both values valid (finite, |v| <= RG_VELOCITY_MAX_ABS)
 * belong to the edge (lo, hi) = (min(a, b), max(a, b)) and add
 *   1                                        to its count (int32)
 *   q(at the hi pixel) - q(at the lo pixel)  to its sum   (int64; exact in any order)
 * Table and totals are those of rg_cell_overlap_i32: open addressing in `workspace` with capacity C = the smallest power of two
 * >= max(2 * max_edges, 64), 64-bit keys lo << 32 | hi (all ones = empty), a slot claimed by one agent-scope relaxed
 * compare-and-swap, linear probing over at most C slots and then totals[1] += 1; nobody waits.  A second launch compacts the
 * occupied slots behind an atomic cursor (totals[0], one atomic per wavefront) into
 *   pair_ids int32 [max_edges][2] = lo, hi;   pair_count int32 [max_edges];   pair_sum int64 [max_edges]
 * in unspecified order; rows at and beyond totals[0] are not written, and slots beyond max_edges are counted but not written.
 * totals int32 [2]: the occupied slots, the insertions that found the table full.  The result is COMPLETE iff
 * totals[0] <= max_edges && totals[1] == 0, and then the SET of (lo, hi, count, sum) is bit-reproducible.  An edge that is
 * written at all carries its full count and sum whatever was dropped (a later insertion of its key always finds its slot).
 * How it runs: one thread per pixel, a wavefront covers 64 consecutive flat indices.  The two directions are taken in turn; a
 * wavefront whose ballot shows no edge in a direction skips it (most do).  Runs of lanes with an equal key are combined with a
 * segmented shuffle scan and only the run's last lane inserts, with one 32-bit and one 64-bit relaxed atomic add: along a border
 * that follows a row, 64 pixel pairs are one insertion.  Values are read only where two regions meet.
 * workspace: 8-byte aligned, rg_region_edges_workspace_bytes(max_edges) = 20 * C bytes (keys, sums, counts), contents
 * undefined before and after.
 * RG_EINVAL before any launch: a null pointer; the sizes; max_edges < 1 or >= 2^30; an output or the workspace overlapping an
 * input.  RG_EALIGN: pair_sum or the workspace not 8-byte aligned.  RG_EWORKSPACE: a workspace too small.  h == 0 or w == 0
 * zeroes totals and returns. */
int64_t rg_region_edges_workspace_bytes(int64_t max_edges);
int rg_region_edges_f32(const float* values, const int32_t* regions, int32_t n_planes, int32_t h, int32_t w, int32_t wrap_rows,
                        int64_t max_edges, int32_t* pair_ids, int32_t* pair_count, int64_t* pair_sum, int32_t* totals,
                        void* workspace, int64_t workspace_bytes, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * 4  Add each region's whole number of Nyquist intervals.
 *
 * fold_lut int32 [n_regions] (may be NULL when n_regions == 0): the fold of region id at fold_lut[id - 1].
 *   f   = fold_lut[regions - 1]
 *   out = (float)((double)v + (double)f * (2.0 * Vn_s))         one float64 multiply, one add, one rounding
 * A gate with regions <= 0 or an id above n_regions gets NaN; any NaN result is the quiet NaN 0x7FC00000.
 * folds (optional int32 [S][R][G]) = f, and 0 where out is NaN.
 * In place: out == vel is allowed (each gate is read before it is written); any other overlap of out or folds with an input or
 * each other is refused.
 * RG_EINVAL before any launch: a null vel, regions, nyquist_host or out; a null fold_lut with n_regions > 0; n_regions < 0; the
 * size limits; a Nyquist velocity out of range; a refused overlap.  G == 0 returns RG_OK without a launch. */
int rg_velocity_apply_folds_f32(const float* vel, const int32_t* regions, const int32_t* fold_lut, int32_t n_regions, int32_t S,
                                int32_t R, int32_t G, const double* nyquist_host, float* out, int32_t* folds,
                                rg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RADARGRID_VELOCITY_H */
