/*
 * radargrid_hip.h -- C ABI of libradargrid_hip.so (MI355X / gfx950 HIP kernels for the radar_grid hot path).
 *
 * The reference (jgmarti84/radar-processor) is pure Python/NumPy: it has no FFI, plugin or operator
 * interface for this path.  The drop-in boundary is therefore the Python function surface of
 * `radar_grid` (src/radar_grid/__init__.py:39-82), and this header is the native layer directly beneath
 * it.  Each entry point names the reference code it replaces (paths relative to /root/reference/).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter name ends in `_host`;
 *   - the caller owns every buffer; no entry point allocates, frees or synchronises;
 *   - all work is enqueued on the caller's `hipStream_t` (passed as void*), so calls are graph-capturable;
 *   - return value: RG_OK (0) or a negative rg_status; rg_last_error() gives a thread-local message;
 *   - float32 device arrays read with 16-byte vector loads must be 16-byte aligned (RG_EALIGN otherwise);
 *   - no global mutable state: entry points are thread-safe per stream.
 *
 * Data layout in HBM
 *   gates      flat ray-major index g = (sweep*n_az + iaz)*n_gates + k   (radar_grid/utils.py:35-37)
 *   voxels     z-major flat index v = (iz*ny + iy)*nx + ix               (radar_grid/compute.py:188-190,257-258)
 *   CSR        indptr[V+1] (int32 or int64), gate_idx int32[P], weights float32[P]  (radar_grid/geometry.py:46-52)
 *   packed fields  float32 [G][stride], stride in {1,2,4,8}: slot f of gate g holds field f's value, or the
 *              EXCLUDED sentinel when the gate is masked/filtered for that field, so that the gather in
 *              rg_csr_apply_f32 needs ONE load per pair for all fields (mask folded into the value).
 */
#ifndef RADARGRID_HIP_H
#define RADARGRID_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version: bumped whenever a signature in this header changes (an argument inserted, a meaning changed).  The Python
 * binding (radar_processor_amd/_native.py: ABI_VERSION) refuses a library whose rg_version() differs, so a stale git-ignored
 * .so is reported as such instead of being called with shifted arguments.  History: 100 rounds 1-2; 101 rec_order / plane0 of
 * rg_csr_compact_pack and rg_csr_compact_apply_packed_f32 (round 3); 102 rg_csr_compact_apply_columns_f32, diagnostic tile
 * codes refused by the product build (round 4); 103 the row-wise kernel of rg_csr_compact_apply_packed_f32 takes 1-8 fields
 * (no signature changed: a 102 library answers RG_EUNSUPPORTED for 5-8); 104 rg_cellgrid.levels + the per-level gate lists
 * (rg_geom_bin_levels_count / rg_geom_bin_gates_levels_f32); still 104: the packed records' two codings -- no signature
 * changed, rg_csr_compact_pack_dense was ADDED (a library without it fails to bind by name) and rg_csr_compact_pack refuses work; the
 * mosaic combine rules -- rg_roi_grid_mosaic_combine_f32 and rg_roi_section_mosaic_combine_f32 were ADDED, no signature changed; the column profile -- rg_column_profile_f32 was ADDED;
 * georeferencing -- rg_gates_to_frame_f32 and rg_frame_to_lonlat_f64 were ADDED; the Web Mercator warp and the overview
 * pyramid -- rg_warp_mercator_f32, rg_warp_mercator_rgba8, rg_overview_f32 and rg_overview_rgba8 were ADDED; connected echo regions -- rg_components_workspace_bytes,
 * rg_label_components_f32, rg_component_stats_f32 and rg_despeckle_select_f32 were ADDED; echo motion and nowcasts --
 * rg_motion_quantize_f32, rg_block_match_u8 and rg_advect_f32 were ADDED; rain rate and accumulation -- rg_rain_rate_f32 and
 * rg_accumulate_advected_f32 were ADDED. */
#define RG_VERSION 104
#define RG_MAX_FIELDS 8

typedef void* rg_stream_t; /* hipStream_t */

typedef enum rg_status {
  RG_OK = 0,
  RG_EINVAL = -1,       /* bad argument (null pointer, negative size, unknown enum) */
  RG_EALIGN = -2,       /* a vector-loaded buffer is not 16-byte aligned */
  RG_ELAUNCH = -3,      /* hipGetLastError() after a launch */
  RG_EWORKSPACE = -4,   /* workspace too small */
  RG_EUNSUPPORTED = -5, /* e.g. n_fields > RG_MAX_FIELDS */
  RG_ENODEVICE = -6     /* no HIP device visible */
} rg_status;

/* Quiet-NaN bit pattern that marks "gate excluded for this field" inside packed fields.  A data NaN that
 * is NOT masked keeps its own payload and propagates like in NumPy (interpolate.py:78-82), with one exception: an
 * unmasked value that carries exactly these bits is stored by rg_pack_fields_f32 as the canonical quiet NaN 0x7FC00000, so
 * that it keeps propagating as a NaN and is never taken for the sentinel. */
#define RG_EXCLUDED_BITS 0x7FD1CE5Du

int rg_version(void);
const char* rg_last_error(void);
/* number of visible HIP devices, or RG_ENODEVICE */
int rg_device_count(void);
/* measurement aid (no reference counterpart): streams `bytes` of `buffer` with 16-byte loads and stores nothing
 * (`sink` = one float the kernel never writes in practice); bench.py times it to report the read bandwidth this
 * GPU delivers to a pure streaming kernel next to the 8 TB/s spec peak (roofline.ceiling_measured). */
int rg_stream_read_probe(const void* buffer, int64_t bytes, float* sink, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * a1  antenna -> Cartesian (PyART antenna_vectors_to_cartesian, call sites radar_grid/utils.py:35-37).
 * float64 math, float32 stores.  x,y,z are [n_rays][n_gates] ray-major.
 * ------------------------------------------------------------------------------------------------- */
int rg_antenna_to_cartesian_f32(const double* ranges_m, int32_t n_gates,
                                const double* az_deg, const double* el_deg, int32_t n_rays,
                                float* x, float* y, float* z, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * a3  GateFilter predicates (radar_grid/filters.py:114-258): mask_inout[g] |= pred(data[g]).
 * NaN compares false, so threshold filters never exclude NaN gates (filters.py:134).  Any non-zero byte of mask_inout
 * counts as set; the kernel ORs 1 into the byte where the predicate holds and leaves the other bits as they are.
 * ------------------------------------------------------------------------------------------------- */
typedef enum rg_gate_op {
  RG_GATE_BELOW = 0,   /* data <  a            filters.py:134 */
  RG_GATE_ABOVE = 1,   /* data >  a            filters.py:157 */
  RG_GATE_BETWEEN = 2, /* a < data < b         filters.py:182 */
  RG_GATE_OUTSIDE = 3, /* data < a || data > b filters.py:207 */
  RG_GATE_EQUAL = 4,   /* |data - a| < b       filters.py:232 */
  RG_GATE_INVALID = 5  /* NaN or Inf           filters.py:257 */
} rg_gate_op;

int rg_gate_mask_f32(const float* data, int64_t n_gates, int32_t op, float a, float b,
                     uint8_t* mask_inout, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * a2/a8 prologue  mask merge (radar_grid/interpolate.py:59-64) folded into the field values.
 *   packed[g*stride + f] = (masks_host[f] && masks_host[f][g]) || (shared_mask && shared_mask[g])
 *                          ? EXCLUDED : fields_host[f][g]          for f <  n_fields
 *                          = EXCLUDED                               for f >= n_fields (padding slots)
 * fields_host / masks_host are HOST arrays of n_fields DEVICE pointers (mask entries may be NULL, and so may masks_host);
 * any non-zero mask byte excludes.  An unmasked value keeps its bits, NaN payloads included -- except the one value whose
 * bits are RG_EXCLUDED_BITS, which is stored as the canonical quiet NaN 0x7FC00000 (see RG_EXCLUDED_BITS).
 * ------------------------------------------------------------------------------------------------- */
int rg_pack_fields_f32(int32_t n_fields, const float* const* fields_host, const uint8_t* const* masks_host,
                       const uint8_t* shared_mask, int64_t n_gates, int32_t stride, float* packed,
                       rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * a8/a9  K1 csr_apply: replaces radar_grid/interpolate.py:69-104 (apply_geometry) and the per-field loop
 * of :137-140 (apply_geometry_multi) with ONE pass over the CSR for all n_fields field-volumes.
 *   out[f*n_vox + v] = sum_j w_j*val_f(g_j) / sum_j w_j   over pairs j of row v whose gate is not EXCLUDED
 *                      for field f, if that weight sum is > 0; otherwise fill_value.
 * Arithmetic: float32 products and float32 sums (as the reference under NumPy >= 2), added in a fixed,
 * launch-independent order (per 64-row segment: tiles of pairs, a few interleaved partial sums per row, combined with
 * wavefront shuffles) -- bit-reproducible run to run, not NumPy's pairwise order; only the final division is done in
 * float64 and rounded to float32.  Worst relative deviation from the reference's grids on the golden fixtures is recorded
 * by tests/test_gpu_parity.py::test_reference_grid_relative_error (a few float32 ulps).
 * the gather goes through a range-checked buffer resource of n_gates * stride * 4 bytes (which must stay below
 * 4 GiB): a gate index outside [0, n_gates) reads as 0.0 and cannot fault the GPU.
 * indptr must be non-decreasing with indptr[0] = 0 and indptr[n_vox] = n_pairs.
 * line_len: rows per grid line (nx of an nz x ny x nx grid; n_vox must be a multiple of it; <= 0 = one line of n_vox
 * rows).  A wavefront owns a segment of up to 64 consecutive rows of ONE line (a line is cut into ceil(line_len / 64)
 * balanced segments); the value only changes which rows share a wavefront -- hence the order of the float32 adds --
 * never which pairs are summed.
 * ------------------------------------------------------------------------------------------------- */
int rg_csr_apply_f32(const void* indptr, int32_t indptr_is_i64, const int32_t* gate_idx, const float* weights,
                     int64_t n_vox, int64_t n_pairs, int64_t line_len,
                     const float* packed, int32_t n_fields, int32_t stride, int64_t n_gates,
                     float fill_value, float* out, rg_stream_t stream);
/* same kernel with the pipeline tile selected explicitly: variant = 0 (what rg_csr_apply_f32 runs) or 128, 192, 256, 320,
 * 384, 512 pairs per step (right answers, another order of the float32 adds; used by the bit-identity tests of the compact
 * kernels).  Anything else is RG_EINVAL. */
int rg_csr_apply_f32_ex(const void* indptr, int32_t indptr_is_i64, const int32_t* gate_idx, const float* weights,
                        int64_t n_vox, int64_t n_pairs, int64_t line_len,
                        const float* packed, int32_t n_fields, int32_t stride, int64_t n_gates,
                        float fill_value, float* out, int32_t variant, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * a11  K3 column reduce: radar_grid/products.py:488-490 (nanmax), :533-535 (nanmin), :578-580 (nanmean)
 * over levels z_lo..z_hi (inclusive, already clipped by the caller as products.py:484-485 does).
 * out_arg (optional, MAX/MIN only): first level attaining the extremum, -1 for an all-NaN column
 * (np.nanargmax order; build-defined).
 * In level order: MAX / MIN start from the first non-NaN level and keep the held value when held >= v (MAX) / held <= v (MIN)
 * or v is NaN, so that the first of equal values -- the sign of a zero included -- is the one stored; MEAN adds the float32
 * values from 0.0f, a NaN counting as 0.0f, and stores (float)((double)sum / (double)count), NaN where count is 0.  The same
 * bits on every launch path (16-byte or one-column accesses, level range split over lanes or not).
 * An EMPTY window (z_lo > z_hi, both inside 0 .. nz-1) is accepted: every value is NaN and every out_arg -1, for all three
 * ops, and nothing of the grid is read.  RG_EINVAL: a null grid / out, nz < 1, n_xy < 0, z_lo < 0, z_hi >= nz, an unknown op,
 * out_arg with RG_COL_MEAN.  n_xy == 0 returns RG_OK.
 * ------------------------------------------------------------------------------------------------- */
typedef enum rg_column_op { RG_COL_MAX = 0, RG_COL_MIN = 1, RG_COL_MEAN = 2 } rg_column_op;

int rg_column_reduce_f32(const float* grid, int32_t nz, int64_t n_xy, int32_t z_lo, int32_t z_hi, int32_t op,
                         float* out, int32_t* out_arg, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * K5  column profile: echo-top and echo-base heights at up to RG_MAX_PROFILE_THRESHOLDS thresholds and the vertically
 * integrated liquid (VIL) of every column, in one bottom-to-top pass over a stored grid.  The reference has none of them:
 * the contract is build-defined (as out_arg above) and stated here; tests/column_profile_oracle.py restates it in float64
 * NumPy.
 *   grid         any [nz][n_xy] stack of float32 planes: n_xy = ny * nx of a lattice grid, or the (nz, 1, n_points) output
 *                of the section entry points;
 *   z_levels     float64 [nz], DEVICE: the height of every level, strictly increasing (the caller checks);
 *   thresholds_host / n_thresholds   0 .. RG_MAX_PROFILE_THRESHOLDS finite thresholds, read on the host and passed by value;
 *   out_top / out_base   float32 [n_thresholds][n_xy] or NULL;  out_vil  float32 [n_xy] or NULL.
 * RG_EINVAL: a null grid or z_levels; all three outputs null; n_thresholds outside 0 .. RG_MAX_PROFILE_THRESHOLDS;
 * n_thresholds == 0 with an out_top or out_base; a non-finite threshold or vil_max_dbz; a window with z_lo < 0, z_hi >= nz
 * or z_lo > z_hi.  n_xy == 0 returns RG_OK.  A launch without VIL reads and writes 16 bytes per lane when n_xy % 4 == 0 and
 * every pointer is 16-byte aligned; otherwise, and with VIL, a lane owns one column -- the same bits either way.
 *
 * The contract, for one column g[] and the levels z_lo .. z_hi only (a level outside the window is never read and never
 * interpolated against); z[] = z_levels, every operation an IEEE float64 operation on the float32 values, unfused:
 *   Echo top at T    k = the highest level of the window with (double)g[k] >= T (a NaN never is); none: NaN.  When
 *                    linear != 0, k < z_hi and g[k] and g[k+1] are both finite:
 *                        z[k] + ((g[k] - T) / (g[k] - g[k+1])) * (z[k+1] - z[k])
 *                    in this association, rounded to float32 once.  In every other case -- k the top of the window, a NaN
 *                    or infinite neighbour, an infinite g[k], linear == 0 -- the result is (float)z[k].
 *   Echo base at T   the mirror image: k = the lowest level with g[k] >= T, the neighbour is k-1 (k > z_lo, both finite):
 *                        z[k] - ((g[k] - T) / (g[k] - g[k-1])) * (z[k] - z[k-1])
 *   VIL (Greene & Clark)   q[k] = 0 where g[k] is NaN, else 10^(min(g[k], vil_max_dbz) / 10);
 *                        VIL = 3.44e-6 * sum_{k = z_lo}^{z_hi - 1} ((q[k] + q[k+1]) / 2)^(4/7) * (z[k+1] - z[k])
 *                    the sum in level order from 0.0, rounded to float32 once; NaN where no level of the window is
 *                    non-NaN, 0.0 for a one-level window that holds a value.  Metres and mm^6 m^-3 in, kg m^-2 out.
 *                    (10^x is the device's float64 exp10, x^(4/7) its exp2(4/7 * log2 x): ~1e-14 relative, so a plane
 *                    agrees with a correctly rounded evaluation to one float32 ulp.)
 * Thresholds are independent of each other: the plane of T is the same bits whether T is asked for alone or with others,
 * on the vector and on the one-column path.
 * ------------------------------------------------------------------------------------------------- */
#define RG_MAX_PROFILE_THRESHOLDS 4
int rg_column_profile_f32(const float* grid, int32_t nz, int64_t n_xy, int32_t z_lo, int32_t z_hi, const double* z_levels,
                          const double* thresholds_host, int32_t n_thresholds, int32_t linear, float* out_top,
                          float* out_base, double vil_max_dbz, float* out_vil, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * a10  K4 CAPPI lerp: radar_grid/products.py:406-412.  out = fl32(fl32(w_lo*lo) + fl32(w_hi*hi)), the
 * float32 arithmetic NumPy >= 2 performs with weak Python-float weights; NaN in either level -> NaN.
 * The scalar control flow (products.py:361-404) stays on the host.
 * ------------------------------------------------------------------------------------------------- */
int rg_cappi_lerp_f32(const float* grid, int64_t n_xy, int32_t k_lo, float w_lo, float w_hi, float* out,
                      rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * a12  constant-elevation PPI: radar_grid/products.py:168-314.  Per pixel the beam height of the elevation
 * (4/3-earth model of products.py:70-87 when earth_curvature != 0, flat earth :164-165 otherwise) selects the
 * altitude; linear != 0 -> float64 lerp between the bracketing levels (`out` is double[ny*nx], products.py:276-309),
 * linear == 0 -> nearest level (`out` is float[ny*nx], products.py:262-272).  The host passes the scalars NumPy
 * evaluates once: cos_clamped = max(cos(elev), 0.01), sin(elev), tan(elev), ke_re = ke * 6371000, ke_re_sq = ke_re**2.
 * xc / yc are the float32 linspace tables of products.py:232-233.
 * ------------------------------------------------------------------------------------------------- */
int rg_elevation_ppi_f32(const float* grid, const float* xc, const float* yc, int32_t nz, int32_t ny, int32_t nx,
                         double cos_clamped, double sin_elev, double tan_elev, double ke_re, double ke_re_sq,
                         double z_min, double z_max, double z_step, int32_t earth_curvature, int32_t linear,
                         void* out, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * a6/a7  geometry builder: replaces radar_grid/compute.py:18-103 (_process_single_level) and the merge of
 * :232-272.  Membership and weights are evaluated in float64 from the float32 inputs with FP contraction
 * disabled, i.e. the reference's arithmetic: valid gate (fl32(z - radar_altitude) <= toa), d2 < r2,
 * r = max(min_radius, sqrt(x^2+y^2+z^2)*beam_factor).
 *
 * Search structure (build-specific): gates are bucketed into a uniform (x,y) cell grid and stably sorted
 * by cell, so every cell row is one contiguous run of `sorted_gates`; a wavefront tests a voxel's runs
 * 64 gates at a time.
 * ------------------------------------------------------------------------------------------------- */
typedef struct rg_cellgrid {
  double x0, y0;         /* lower corner of cell (0,0) */
  double inv_cx, inv_cy; /* 1 / cell size */
  double z_lo, z_hi;     /* gates with z_rel outside [z_lo, z_hi] cannot reach any voxel and are dropped */
  int32_t ncx, ncy;
  int32_t levels;        /* 0 / 1: one list for all grid levels (cell_start[ncx*ncy + 1]); nz: one list PER LEVEL, holding only the
                          * gates that can reach that level (rg_geom_bin_gates_levels_f32; cell_start[nz*ncx*ncy + 1], the cells
                          * of level iz at iz*ncx*ncy ..) -- a third of the candidates per voxel block */
  int32_t level0;        /* per-level lists: the grid level the call's zc[0] is (a call may cover levels level0 .. level0 + nz - 1
                          * of the binned grid by passing zc + level0); 0 otherwise */
} rg_cellgrid;

typedef struct rg_gate4 { float x, y, z; int32_t index; } rg_gate4; /* 16 bytes: one dwordx4 per candidate */

/* RG_W_NEAREST is the reference's 'nearest' = uniform mean over the ROI (radar_grid/compute.py:86-87).
 * RG_W_CLOSEST (rg_roi_grid_f32 only) takes the value of the single closest non-excluded gate inside the ROI -- the
 * selection rule of PyART's map_gates_to_grid(weighting_function='nearest') that radar_processor/processor.py:152-163
 * uses behind the 3-D grid cache; PyART is not in the reference tree, so this mode is parity-unpinned.  Its contract:
 * membership is the float64 `d2 < r2` of every mode; among the member gates the field does not exclude, the smallest float32
 * d2 = fmaf(dz,dz,fmaf(dy,dy,dx*dx)) wins and bit-equal d2 go to the LOWER gate index; the winner's value is stored bit for
 * bit (as packed: a value carrying the bits of RG_EXCLUDED_BITS arrives as the canonical quiet NaN, the one exception),
 * fill_value where there is none.  To float64 the winner is at most (1 + 5u)/(1 - 5u), u = 2^-24, farther (in d2) than
 * the nearest member (oracle.closest_gate_choice derives it; tests/test_gpu_closest.py checks every voxel). */
typedef enum rg_weighting { RG_W_BARNES2 = 0, RG_W_CRESSMAN = 1, RG_W_NEAREST = 2, RG_W_CLOSEST = 3 } rg_weighting;

/* bytes of scratch rg_geom_bin_gates_f32 needs for n_gates gates */
int64_t rg_geom_bin_workspace_bytes(int64_t n_gates, int32_t ncx, int32_t ncy);

/* sorted_gates[0 .. n_binned) in (cell, gate index) order (buffer of n_gates records);
 * cell_start[ncx*ncy + 1], with cell_start[ncx*ncy] = n_binned = number of gates that were kept */
int rg_geom_bin_gates_f32(const float* gate_x, const float* gate_y, const float* gate_z, int64_t n_gates,
                          float radar_altitude, float toa, const rg_cellgrid* cells_host,
                          rg_gate4* sorted_gates, int32_t* cell_start,
                          void* workspace, int64_t workspace_bytes, rg_stream_t stream);

/* Per-level lists: a gate g that rg_geom_bin_gates_f32 would keep is listed under level iz when |z_rel(g) - zc[iz]| <= R_g,
 * R_g = max(min_radius, beam_factor * |g| / (1 - beam_factor)), and under no level beyond the inflated bound
 * (1 + 1e-6) * R_g + 1 mm (the inflation covers the rounding of this very computation) -- R_g bounds the radius of influence
 * of ANY voxel the gate can be a neighbour of (compute.py:46-47: r_v = max(min_radius, |v| * beam_factor) and
 * |v| <= |g| + r_v), so no neighbour is lost; needs 0 <= beam_factor < 0.5 and min_radius >= 0 (RG_EUNSUPPORTED otherwise:
 * use the single list).  rg_geom_bin_levels_count writes the number of (gate, level) entries to *total (device memory);
 * rg_geom_bin_gates_levels_f32 then fills sorted_gates[n_entries] in (level, cell, gate index) order and
 * cell_start[nz*ncx*ncy + 1] (cells->levels must equal nz).  n_entries must be the total rg_geom_bin_levels_count returned
 * for the same arguments: it sizes the buffers and is not re-checked.  zc: the float32 level coordinates (device). */
int rg_geom_bin_levels_count(const float* gate_x, const float* gate_y, const float* gate_z, int64_t n_gates,
                             float radar_altitude, float toa, const rg_cellgrid* cells_host, const float* zc, int32_t nz,
                             double min_radius, double beam_factor, int64_t* total, rg_stream_t stream);
int64_t rg_geom_bin_levels_workspace_bytes(int64_t n_gates, int64_t n_entries, int64_t n_cells_total);
int rg_geom_bin_gates_levels_f32(const float* gate_x, const float* gate_y, const float* gate_z, int64_t n_gates,
                                 float radar_altitude, float toa, const rg_cellgrid* cells_host, const float* zc, int32_t nz,
                                 double min_radius, double beam_factor, int64_t n_entries, rg_gate4* sorted_gates,
                                 int32_t* cell_start, void* workspace, int64_t workspace_bytes, rg_stream_t stream);

/* counts[v] = number of gates within voxel v's radius of influence; xc/yc/zc are the float32 linspace
 * coordinate tables of radar_grid/compute.py:184-186 (device pointers). */
int rg_geom_count_f32(const rg_gate4* sorted_gates, const int32_t* cell_start, const rg_cellgrid* cells_host,
                      const float* xc, const float* yc, const float* zc, int32_t nz, int32_t ny, int32_t nx,
                      double min_radius, double beam_factor, int32_t* counts, rg_stream_t stream);

/* indptr[0..n] = exclusive prefix sum of counts[0..n) widened to int64 (indptr[n] = total pairs) */
int64_t rg_scan_workspace_bytes(int64_t n);
int rg_scan_counts_i64(const int32_t* counts, int64_t n, int64_t* indptr, void* workspace,
                       int64_t workspace_bytes, rg_stream_t stream);

/* second pass: writes gate_idx / weights of every row at indptr[v].. in (cell row, gate index) order */
int rg_geom_fill_f32(const rg_gate4* sorted_gates, const int32_t* cell_start, const rg_cellgrid* cells_host,
                     const float* xc, const float* yc, const float* zc, int32_t nz, int32_t ny, int32_t nx,
                     double min_radius, double beam_factor, int32_t weighting, const int64_t* indptr,
                     int32_t* gate_idx, float* weights, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * K2  fused on-the-fly gridding: the neighbour search of rg_geom_count/fill_f32 fused with the masked
 * weighted mean of rg_csr_apply_f32 -- radar_grid/compute.py:46-91 + radar_grid/interpolate.py:69-104 in
 * one kernel, no CSR in memory (for grids whose pair count makes the CSR pointless or impossible,
 * SURVEY.md F6).  Same neighbour sets as the builder, weights evaluated in float32 (|rel err| < 2e-6 vs the builder's
 * float64-exact ones), float32 sums per voxel lane; results differ from the CSR path by that and by summation order.  `packed` is the rg_pack_fields_f32 layout over the same gate numbering as the
 * gates that were binned.
 * ------------------------------------------------------------------------------------------------- */
int rg_roi_grid_f32(const rg_gate4* sorted_gates, const int32_t* cell_start, const rg_cellgrid* cells_host,
                    const float* xc, const float* yc, const float* zc, int32_t nz, int32_t ny, int32_t nx,
                    double min_radius, double beam_factor, int32_t weighting,
                    const float* packed, int32_t n_fields, int32_t stride, float fill_value, float* out,
                    rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Several radars on one grid (mosaic): K2 over up to RG_MAX_RADARS search structures in one launch, the joint masked
 * weighted mean
 *     out[f][v] = sum_r sum_{live j} w_j * v_j / sum_r sum_{live j} w_j   (fill_value where the sum is not > 0)
 * where radar r's neighbours and weights of voxel v are those of radar_grid/compute.py:46-91 evaluated in that radar's
 * frame (voxel coordinates relative to its antenna), and the mean is radar_grid/interpolate.py:69-104 over the union of
 * every radar's neighbours.  The reference has no joint mean: it grids one radar per geometry.  Per radar, the
 * arithmetic is rg_roi_grid_f32's; hits of all radars add into the same float32 accumulators, radar by radar in table
 * order, and a radar whose window misses a voxel block is skipped.  One entry built from a search structure with a
 * full-grid window and gate_offset 0 returns exactly the bits of rg_roi_grid_f32 on that structure.
 *
 * Entry r describes radar r:
 *   sorted_gates, cell_start, cells   its cell-sorted gates (rg_geom_bin_gates_f32 / _levels_f32); a gate's index is the
 *                                     radar's OWN gate number;
 *   xc, yc, zc                        the float32 coordinates relative to this radar of the window's columns (xc[nx_win]),
 *                                     rows (yc[ny_win]) and of every grid level (zc[nz]) -- slices of the radar's full
 *                                     tables, so that they round as those do;
 *   ix0, iy0, nx_win, ny_win          the window: voxels ix0 .. ix0 + nx_win - 1, iy0 .. iy0 + ny_win - 1 of the shared
 *                                     grid (all levels); nx_win or ny_win == 0: the radar reaches no voxel (its pointers
 *                                     are not read);
 *   gate_offset, n_gates              radar r's gate g is packed slot gate_offset + g of `packed` (the rg_pack_fields_f32
 *                                     layout over the concatenated gates); gate_offset + n_gates <= n_gates_total.
 * The table is read on the host and passed by value in the kernel arguments.  RG_W_CLOSEST is not supported.
 * ------------------------------------------------------------------------------------------------- */
#define RG_MAX_RADARS 16
typedef struct rg_mosaic_radar {
  const rg_gate4* sorted_gates;
  const int32_t* cell_start;
  rg_cellgrid cells;
  const float *xc, *yc, *zc;
  int32_t ix0, iy0, nx_win, ny_win;
  int64_t gate_offset, n_gates;
} rg_mosaic_radar;

int rg_roi_grid_mosaic_f32(const rg_mosaic_radar* radars_host, int32_t n_radars, int32_t nz, int32_t ny, int32_t nx,
                           double min_radius, double beam_factor, int32_t weighting, const float* packed,
                           int32_t n_fields, int32_t stride, int64_t n_gates_total, float fill_value, float* out,
                           rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * How a mosaic combines its radars: rg_roi_grid_mosaic_combine_f32 and rg_roi_section_mosaic_combine_f32 take the
 * arguments of rg_roi_grid_mosaic_f32 / rg_roi_section_mosaic_f32 plus `combine` and `out_radar`, check them as those do
 * (RG_W_CLOSEST stays RG_EUNSUPPORTED) and refuse an unknown combine code with RG_EINVAL.
 *
 * For field f and voxel (or section sample) v, radar k of the call's table HAS A VALUE when its own live weight sum is
 * > 0; its value m_k is exactly what the mean entry point stores for a table holding only entry k -- the same arithmetic in
 * the same order, from sums that start at zero when the radar's visit starts.
 *   RG_COMBINE_MEAN           the joint mean: the bits of rg_roi_grid_mosaic_f32 / rg_roi_section_mosaic_f32.
 *   RG_COMBINE_MAX            walk the table in order; radar k takes over when nothing is held yet, or m_k > held, or the
 *                             held value is NaN and m_k is not.  Equal values, and -0.0 against +0.0, stay with the earlier
 *                             table position.
 *   RG_COMBINE_NEAREST_RADAR  among the radars that have a value, the one with the smallest D_k = x*x + y*y + z*z, in
 *                             float64, unfused, from the float32 coordinates of v in radar k's frame (the expression under
 *                             the square root of the radius of influence); equal D goes to the earlier table position.  A
 *                             radar whose window misses v -- whose point is NaN -- has no value there.
 * The winner's bits are copied, never computed with.  No radar has a value: fill_value.  The choice is per field (masks
 * are per field).
 * out_radar (may be null): uint8 [n_fields][n_samples], the table position of the radar that supplied the value, 255 where
 * the value is the fill.  With RG_COMBINE_MEAN a non-null out_radar is RG_EINVAL.
 * ------------------------------------------------------------------------------------------------- */
typedef enum rg_combine { RG_COMBINE_MEAN = 0, RG_COMBINE_MAX = 1, RG_COMBINE_NEAREST_RADAR = 2 } rg_combine;

int rg_roi_grid_mosaic_combine_f32(const rg_mosaic_radar* radars_host, int32_t n_radars, int32_t nz, int32_t ny,
                                   int32_t nx, double min_radius, double beam_factor, int32_t weighting,
                                   const float* packed, int32_t n_fields, int32_t stride, int64_t n_gates_total,
                                   float fill_value, float* out, int32_t combine, uint8_t* out_radar, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Vertical cross-section along any path: K2's arithmetic at n_points sample columns (xs[i], ys[i]) -- float32 metres in
 * the radar frame, device pointers; not necessarily equally spaced, sorted or distinct -- times the nz levels of zc.
 * Sample (k, i) is what radar_grid/compute.py:46-91 + radar_grid/interpolate.py:69-104 would put into a voxel lying exactly
 * at (xs[i], ys[i], zc[k]); out is float32 [n_fields][nz][n_points], row k * n_points + i the row order of a grid of shape
 * (nz, 1, n_points).  The search structure is the one of the lattice entry points; every point must lie inside the xy
 * rectangle it was built for (the caller checks: the points are device memory).  A point with a non-finite coordinate
 * has no neighbours.  Weights of rg_roi_section_f32 as rg_roi_grid_f32's (same budgets); rg_section_count_f32 /
 * rg_section_fill_f32 are the builder passes (row lengths; gate index and float64-exact weight rounded to float32, as
 * rg_geom_fill_f32 writes them; rg_scan_counts_i64 in between).  RG_W_CLOSEST is not supported (RG_EUNSUPPORTED).
 * ------------------------------------------------------------------------------------------------- */
int rg_roi_section_f32(const rg_gate4* sorted_gates, const int32_t* cell_start, const rg_cellgrid* cells_host,
                       const float* xs, const float* ys, const float* zc, int32_t nz, int32_t n_points,
                       double min_radius, double beam_factor, int32_t weighting,
                       const float* packed, int32_t n_fields, int32_t stride, float fill_value, float* out,
                       rg_stream_t stream);
int rg_section_count_f32(const rg_gate4* sorted_gates, const int32_t* cell_start, const rg_cellgrid* cells_host,
                         const float* xs, const float* ys, const float* zc, int32_t nz, int32_t n_points,
                         double min_radius, double beam_factor, int32_t* counts, rg_stream_t stream);
int rg_section_fill_f32(const rg_gate4* sorted_gates, const int32_t* cell_start, const rg_cellgrid* cells_host,
                        const float* xs, const float* ys, const float* zc, int32_t nz, int32_t n_points,
                        double min_radius, double beam_factor, int32_t weighting, const int64_t* indptr,
                        int32_t* gate_idx, float* weights, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * A vertical cross-section through a mosaic: rg_roi_section_f32 over up to RG_MAX_RADARS search structures in one launch,
 *     out[f][k * n_points + i] = sum_r sum_{live j} w_j * v_j / sum_r sum_{live j} w_j   (fill_value where the sum is not > 0)
 * where radar r's neighbours and weights of sample (k, i) are those of radar_grid/compute.py:46-91 at (xs_r[i], ys_r[i],
 * zc_r[k]) -- the point and the level in radar r's frame -- and the mean is radar_grid/interpolate.py:69-104 over the union
 * of every radar's neighbours.  Per radar the arithmetic is rg_roi_section_f32's; hits of all radars add into the same
 * float32 accumulators, radar by radar in table order.  One entry with gate_offset 0 returns exactly the bits of
 * rg_roi_section_f32 on the same search structure and points.
 *
 * Entry r describes radar r:
 *   sorted_gates, cell_start, cells   its cell-sorted gates; a gate's index is the radar's OWN gate number;
 *   xs, ys                            float32 [n_points], device: the points relative to this radar.  A point the radar
 *                                     cannot serve (outside the rectangle its search structure was built for) carries a
 *                                     NaN: it has no neighbours among this radar's gates.  A block of 4 consecutive points
 *                                     without a live one reads nothing of the radar's search structure;
 *   zc                                float32 [nz], device: the levels relative to this radar;
 *   gate_offset, n_gates              radar r's gate g is packed slot gate_offset + g of `packed`;
 *                                     gate_offset + n_gates <= n_gates_total.
 * An entry with n_gates == 0 or a null sorted_gates takes no part: none of its pointers is read.  The table is read on
 * the host and passed by value in the kernel arguments.  RG_W_CLOSEST is not supported (RG_EUNSUPPORTED).
 * ------------------------------------------------------------------------------------------------- */
typedef struct rg_section_radar {
  const rg_gate4* sorted_gates;
  const int32_t* cell_start;
  rg_cellgrid cells;
  const float *xs, *ys, *zc;
  int64_t gate_offset, n_gates;
} rg_section_radar;

int rg_roi_section_mosaic_f32(const rg_section_radar* radars_host, int32_t n_radars, int32_t nz, int32_t n_points,
                              double min_radius, double beam_factor, int32_t weighting, const float* packed,
                              int32_t n_fields, int32_t stride, int64_t n_gates_total, float fill_value, float* out,
                              rg_stream_t stream);
/* ... with a combine rule (rg_combine, above): sample (k, i) is row k * n_points + i of out and of out_radar */
int rg_roi_section_mosaic_combine_f32(const rg_section_radar* radars_host, int32_t n_radars, int32_t nz, int32_t n_points,
                                      double min_radius, double beam_factor, int32_t weighting, const float* packed,
                                      int32_t n_fields, int32_t stride, int64_t n_gates_total, float fill_value, float* out,
                                      int32_t combine, uint8_t* out_radar, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * (f)3  processor-style collapse of the cached 3-D grid to the 2-D product plane:
 * radar_processor/processor.py:480-551 (collapse_grid_to_2d) and radar_processor/utils.py:336-387
 * (collapse_field_3d_to_2d).  'cappi' (nearest level, :530-533) and 'colmax' (:534-535) are
 * rg_column_reduce_f32 over one level / all levels; 'ppi' (:512-528) is the entry below: per pixel
 * r = sqrt(x^2 + y^2), z_target = r*sin_elev + r^2 / two_re (two_re = 2 * 8.49e6 m), level = first argmin of
 * |z_target - z[k]|, all in float64 as NumPy evaluates it; out[p] = grid[level][p].  The host passes
 * sin_elev = sin(deg2rad(elevation)).  x[nx], y[ny], z[nz] are float64 device tables.  out_level may be NULL.
 * A masked voxel is a NaN (the cache package is masked_invalid data).
 * ------------------------------------------------------------------------------------------------- */
int rg_collapse_ppi_f32(const float* grid, const double* x, const double* y, const double* z, int32_t nz, int32_t ny,
                        int32_t nx, double sin_elev, double two_re, float* out, int32_t* out_level,
                        rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * (f)3  threshold masks on a 2-D plane: the re-mask of collapse_grid_to_2d (processor.py:541-546:
 * masked_less_equal / masked_less against vmin) and _apply_filter_masks (processor.py:802-886: visual filters on
 * the plotted field, cross-field and QC filters on cached QC planes), all OR-ed in one pass.  A test drops pixel p
 * when  q < lo (RG_TEST_LO),  q <= lo (RG_TEST_LO | RG_TEST_LO_INCLUSIVE),  q > hi (RG_TEST_HI)  or q is +-inf / NaN
 * (RG_TEST_NONFINITE, the np.ma.masked_invalid of processor.py:541), with
 * q = plane[p] (or src[p] when plane is NULL), compared in float32 as NumPy compares a float32 array with a Python
 * float; NaN never compares true.  A pixel counts as already masked when src_mask[p] != 0 or, without a src_mask,
 * when src[p] is NaN.  out[p] = dropped or masked ? NaN : src[p]  (NULL to skip); out_mask[p] = dropped or masked
 * (NULL to skip).  `tests` is a HOST
 * array of at most RG_MAX_PLANE_TESTS entries whose plane pointers are device pointers.
 * ------------------------------------------------------------------------------------------------- */
#define RG_MAX_PLANE_TESTS 12
typedef enum rg_plane_test_flags {
  RG_TEST_LO = 1, RG_TEST_HI = 2, RG_TEST_LO_INCLUSIVE = 4, RG_TEST_NONFINITE = 8
} rg_plane_test_flags;
typedef struct rg_plane_test {
  const float* plane; /* NULL: test the source plane itself */
  float lo, hi;
  int32_t flags;
} rg_plane_test;

int rg_plane_filter_f32(const float* src, const uint8_t* src_mask, int64_t n, const rg_plane_test* tests,
                        int32_t n_tests, float* out, uint8_t* out_mask, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * (f)4  colormap -> RGBA uint8: radar_grid/geotiff.py:70-145 (apply_colormap_to_array), i.e. matplotlib's
 * Normalize(vmin, vmax, clip=True) followed by Colormap.__call__ and (rgba * 255).astype(uint8).
 *
 * rg_nan_minmax: over the pixels that are not no-data (no-data = equal to `fill` when has_fill, NaN otherwise)
 * out[0] = min and out[1] = max ignoring NaN, out[2] = how many such non-NaN pixels there are, out[3] = how many
 * pixels are not no-data (geotiff.py:111-125: np.nanmin / np.nanmax of valid_data and len(valid_data)); +inf / -inf /
 * 0 when there are none.  `data` is float32 or float64 (data_is_f64), `workspace` needs RG_MINMAX_WORKSPACE_BYTES,
 * out is double[4] on the device.  The comparison with `fill` is made in the data's dtype (float32 data: against (float)fill),
 * so a NaN pixel is no-data only without a fill value; with one it is kept (out[3]) and not counted (out[2]).  n == 0 (data may
 * then be NULL) yields +inf, -inf, 0, 0.
 *
 * rg_colormap_rgba: per pixel v = minimum(maximum(x, vmin), vmax); v -= vmin; v /= (vmax - vmin); v *= n_lut;
 * v == n_lut -> n_lut - 1; index = trunc(v), or n_lut (under) when v < 0, n_lut + 1 (over) when v >= n_lut,
 * n_lut + 2 (bad) when NaN; rgba = lut[index]; alpha = 0 where x is no-data (NaN, or == fill when has_fill; the
 * comparison with fill is made in the data's dtype).  The arithmetic runs in float64 for float32 and float64 data
 * alike: Normalize stores its limits as Python floats, so np.clip promotes a float32 array to float64 before the
 * in-place operations (matplotlib 3.10 / NumPy 2).  vmin == vmax selects entry 0 for every pixel (Normalize fills 0);
 * vmin > vmax is RG_EINVAL.  lut: uint8 [n_lut + 3][4] on the device = (colormap table * 255) truncated,
 * n_lut <= RG_MAX_LUT.  out: uint8 [n][4].
 * ------------------------------------------------------------------------------------------------- */
#define RG_MINMAX_WORKSPACE_BYTES 32768
#define RG_MAX_LUT 4093
int rg_nan_minmax(const void* data, int32_t data_is_f64, int64_t n, int32_t has_fill, double fill, void* workspace,
                  double* out, rg_stream_t stream);
int rg_colormap_rgba(const void* data, int32_t data_is_f64, int64_t n, double vmin, double vmax, int32_t has_fill,
                     double fill, const uint8_t* lut, int32_t n_lut, uint8_t* out, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * GridFilter (radar_grid/filters.py:609-780): value filters on a product plane after interpolation.
 * out[p] = hit(p) ? fill_value : src[p]  with  hit = (flags & RG_TEST_LO and v < lo) or (flags & RG_TEST_HI and v > hi)
 * or (flags & RG_TEST_NONFINITE and v is NaN / +-inf) or (mask != NULL and mask[p] != 0); comparisons in the
 * plane's dtype (float32 when data_is_f64 == 0, as NumPy compares a float32 array with a Python float), so a NaN
 * pixel is only ever replaced by the NONFINITE test or the mask.  src == out is allowed.
 * ------------------------------------------------------------------------------------------------- */
int rg_grid_filter(const void* src, int32_t data_is_f64, int64_t n, int32_t flags, double lo, double hi,
                   const uint8_t* mask, double fill_value, void* out, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * K1c  csr_apply over a compact device copy of the CSR -- same results as rg_csr_apply_f32 for every field count,
 * bit for bit, from 6 instead of 8 streamed bytes per pair and one gather per DISTINCT gate of a chunk instead of one
 * per pair.  (Its packed form, rg_csr_compact_apply_packed_f32 below, is the faster one where the weights allow it.)  The grid is planes x lines x rows (n_vox = n_planes * lines_per_plane * line_len; nz x ny x nx for a radar
 * grid).  A chunk is a 2-D patch: segment sx (one of the ceil(line_len / 64) balanced pieces of a line, the unit one
 * wavefront of rg_csr_apply_f32 owns) of the RG_COMPACT_LINES consecutive lines yg*RG_COMPACT_LINES.. of one plane; chunks are
 * numbered c = (plane * ceil(lines_per_plane / RG_COMPACT_LINES) + yg) * ceil(line_len / 64) + sx.  Chunk c lists its
 * distinct gate indices in dict[dict_ptr[c] .. dict_ptr[c+1]) (at most 65536 of them, any order) and pair p of one of
 * its rows stores local_idx[p] = position of its gate in that list.  A chunk with MORE distinct gates is stored split:
 * dict[dict_ptr[c] + w], w < RG_COMPACT_LINES, is the offset (from dict_ptr[c]) of a dictionary of its own for line w's
 * segment, and positions refer to that; such a chunk is recognised by dict_ptr[c+1] - dict_ptr[c] > 65536.
 * indptr and weights are those of the standard CSR
 * (radar_grid/geometry.py:46-52), which stays the interchange format; the compact arrays are derived from it on the
 * device (radar_processor_amd/grid_geometry.py: CompactCSR).  `packed` / n_fields / stride: as rg_csr_apply_f32.
 * window_cap: how many dictionary entries (of `stride` floats) a workgroup keeps in LDS (<= RG_COMPACT_MAX_WINDOW,
 * clamped to what fits next to the kernel's own LDS); chunks with a longer dictionary gather per pair from memory, so
 * any value is correct and the choice only affects speed.  tile: pairs per pipeline step, 0 = default (= the tile of
 * rg_csr_apply_f32 for the same field count; other values change the order of the float32 adds); any other tile is
 * RG_EINVAL.
 * line_len <= 0 means one line of n_vox rows, lines_per_plane <= 0 one plane.
 * ------------------------------------------------------------------------------------------------- */
#ifndef RG_COMPACT_LINES
#define RG_COMPACT_LINES 4
#endif
#define RG_COMPACT_MAX_WINDOW 8192
/* Block -> chunk map of the apply kernels: block b = (line group grp, column col) takes chunk column
 * (col + (grp * RG_COMPACT_ROTATION) mod nsx) mod nsx of its line group (grp counted through all planes, 32-bit unsigned
 * arithmetic), so that every XCD sees every column of the grid.  Part of the record layout when the records are stored
 * in dispatch order (below). */
#define RG_COMPACT_ROTATION 5
int rg_csr_compact_apply_f32(const void* indptr, int32_t indptr_is_i64, const uint16_t* local_idx, const float* weights,
                             const int64_t* dict_ptr, const int32_t* dict, int64_t n_vox, int64_t n_pairs,
                             int64_t line_len, int64_t lines_per_plane, const float* packed, int32_t n_fields,
                             int32_t stride, int64_t n_gates, float fill_value, float* out, int32_t window_cap,
                             int32_t tile, rg_stream_t stream);

/* Packed pair stream of the compact copy: positions and weights of three consecutive pairs of a segment in one record,
 * streamed with one aligned 16-byte load per lane.  The coding of a chunk's records follows from the size of its dictionary
 * (dict_ptr[chunk + 1] - dict_ptr[chunk]), which every reader has at hand:
 *   WIDE, more than RG_DENSE_MAX_DICT entries: 16 bytes, 16-bit positions, 5.33 bytes per pair; record q at byte 16 * q
 *     record = [w0:26 | p2 bits 0-5] [w1:26 | p2 bits 6-11] [w2:26 | p2 bits 12-15] [p0:16 | p1:16]   (4 x uint32)
 *   DENSE, at most RG_DENSE_MAX_DICT entries: 14 bytes, 11-bit positions, 4.67 bytes per pair; record q at byte 14 * q of
 *     its segment's records.  M1 = w0:26 | p1 bits 0-5, M2 = w1:26 | p2 bits 0-5, W2 = w2:26 | p2 bits 6-10, P = p0:11 |
 *     p1 bits 6-10 (16 bits), stored as little-endian halfwords
 *       q even: W2.lo W2.hi M1.lo M1.hi M2.lo M2.hi P        q odd: W2.lo M1.lo M1.hi M2.lo M2.hi W2.hi P
 *     so that the aligned 16 bytes at (14 * q) & ~3 hold M1 and M2 in dwords 1 and 2 whatever the parity of q, and W2 and
 *     P come out of dwords 0 and 3 with one funnel shift by 16 * (q & 1) (csrc/rg_compact_layout.hpp: rec_decode /
 *     rec_encode_dense).
 * rec_ptr counts 16-byte UNITS: every segment starts on a 16-byte boundary and takes n units (wide) or ceil(14 * n / 16)
 * units (dense) for its n = ceil(pairs / 3) records.
 *   weight code = float32 bits of the weight - w_base; w_base has its low 26 bits clear (an exponent that is a multiple of
 *   8, shifted left by 23), so adding it back is an OR; the caller guarantees that every code fits 26 bits (all weights
 *   positive, exponents w_base >> 23 .. (w_base >> 23) + 7), which makes the coding lossless.
 * A segment (the <= 64 rows one wavefront owns) holds ceil(pairs / 3) records, fewer than 2^27; where they lie is
 * rec_order's business -- rec_ptr[s] .. rec_ptr[s+1] are the records of the segment in SLOT s:
 *   RG_REC_ORDER_SEGMENT   s = seg = line * ceil(line_len / 64) + sx (line-major; rec_ptr has segments + 1 entries);
 *   RG_REC_ORDER_DISPATCH  s = b * RG_COMPACT_LINES + w for the segment wavefront w of block b reads (block -> chunk map:
 *                          RG_COMPACT_ROTATION above; rec_ptr has chunks * RG_COMPACT_LINES + 1 entries, slots of lines
 *                          past the end of a plane are empty).  The four segments of a workgroup are then neighbours in
 *                          the stream and consecutive workgroups read consecutive stretches of it: whatever the physical
 *                          placement of the array, the launch reads it as ONE moving front.
 * rec_ptr is built by the caller.  rg_csr_compact_pack_dense fills `records` from local_idx + weights (error_flag: 1 = rec_ptr
 * inconsistent with indptr, 2 = a weight outside the code, 4 = a segment with 2^27 records or more); for a slab of whole
 * planes of a larger grid pass the slab's indptr / n_rows, rec_ptr + the slab's first slot and plane0 = its first plane.
 * rg_csr_compact_apply_packed_f32 grids 1-8 fused fields (row-wise kernel; the tile kernel over the records: 1-4) through
 * the records (interpolate.py:69-104 / :137-140, the same masked weighted mean as rg_csr_apply_f32: float32 products and sums,
 * float64 only in the final division):
 *   tile = 0    the ROW-WISE kernel: the lanes of a row read the row's records straight from memory and sum them in
 *               registers (no LDS tile), L = 2^k lanes per row chosen per segment from its mean row length.  The order
 *               of the float32 adds is fixed by the geometry and the field count alone (reproducible run to run, on any
 *               window_cap), but it is not the order of rg_csr_apply_f32: the two agree to float32 rounding (the bar of
 *               the parity tests: 1e-5 relative + 1e-5 * max|field|), not bit for bit.  This is the fast path:
 *               1.0-1.5 ms for 1-4 fields on BASELINE config 2 where the tile kernels need 1.1-3.3 ms.  Five to eight
 *               fields (stride 8; eight volumes of one geometry in ONE pass over the records: 15.5 ms on the bench grid
 *               against 2 x 10.5 for two passes of four) keep 40 bytes of LDS per window entry: worth it where the
 *               geometry's window is <= 768 entries (the Python layer decides: gridding.fields_per_pass).
 *   tile = 384  the TILE kernel of rg_csr_compact_apply_f32 over the same records: the results of rg_csr_apply_f32 for the
 *               same fields, bit for bit.
 *   tile = 2000 + h   row-wise with a diagnostic lane split: h = 1, 2, 4 .. 64 lanes per row, or h = 71 .. 99 = 70 + t to
 *               aim for t records per lane and row (another split = another order of the adds; right answers).
 *   Any other tile is RG_EINVAL.
 * window_cap as for rg_csr_compact_apply_f32; the row-wise kernel keeps one entry more (an all-EXCLUDED sentinel). */
#define RG_REC_ORDER_SEGMENT 0
#define RG_REC_ORDER_DISPATCH 1
#define RG_DENSE_MAX_DICT 2048
/* rg_csr_compact_pack_dense is the packer: rg_csr_compact_pack's arguments plus `dict_ptr` ([chunks + 1] of the grid -- or
 * of the slab -- the row pointers describe; only the differences of neighbouring entries are read), from which it takes
 * every chunk's coding.  rg_csr_compact_pack itself knows no dictionary sizes and therefore cannot choose a coding: it is
 * kept for binary compatibility and returns RG_EUNSUPPORTED whenever there is something to pack. */
int rg_csr_compact_pack_dense(const void* indptr, int32_t indptr_is_i64, const uint16_t* local_idx, const float* weights,
                              int64_t n_rows, int64_t line_len, int64_t lines_per_plane, const int64_t* dict_ptr,
                              const int64_t* rec_ptr, int32_t rec_order, int64_t plane0, uint32_t w_base, void* records,
                              int32_t* error_flag, rg_stream_t stream);
int rg_csr_compact_pack(const void* indptr, int32_t indptr_is_i64, const uint16_t* local_idx, const float* weights,
                        int64_t n_rows, int64_t line_len, int64_t lines_per_plane, const int64_t* rec_ptr,
                        int32_t rec_order, int64_t plane0, uint32_t w_base, void* records, int32_t* error_flag,
                        rg_stream_t stream);
int rg_csr_compact_apply_packed_f32(const void* indptr, int32_t indptr_is_i64, const void* records,
                                    const int64_t* rec_ptr, int32_t rec_order, uint32_t w_base, const int64_t* dict_ptr,
                                    const int32_t* dict, int64_t n_vox, int64_t n_pairs, int64_t line_len,
                                    int64_t lines_per_plane, const float* packed, int32_t n_fields, int32_t stride,
                                    int64_t n_gates, float fill_value, float* out, int32_t window_cap, int32_t tile,
                                    rg_stream_t stream);

/* The ROW-END TABLE of a grid's row pointers, derived data built once per geometry: row_end16[v] = indptr[v + 1] -
 * indptr[r0], the end of row v among the pairs of its segment (r0 = the segment's first row; segments as above: the balanced
 * cuts of a line).  A segment of about 4 600 pairs needs no 8-byte row pointers to say where its rows begin: with the table
 * the row-wise kernel reads 2 bytes per row instead of indptr[v] and indptr[v + 1], and no indptr at all.  A segment whose
 * span exceeds RG_ROW_END16_MAX holds RG_ROW_END16_WIDE in every entry (the kernel tests the last one, once per wavefront)
 * and keeps reading indptr.  rg_csr_row_ends16 writes the table of n_rows rows (int32 or int64 indptr; for a slab of whole
 * planes pass the slab's indptr, n_rows and row_end16 + the slab's first row: an entry depends on its own segment alone).
 * The _ex variants of the three entry points over the packed records take the table as their argument before `stream`;
 * NULL = no table, every segment reads indptr -- which is exactly what the entry points without _ex do.  Same bits either
 * way: the table hands the kernel the same integers.  All of them (with or without a table) leave a chunk without a record
 * -- rec_ptr equal at both ends of the workgroup's RG_COMPACT_LINES slots, RG_REC_ORDER_DISPATCH, grid mode -- as soon as
 * its rows hold fill_value. */
#define RG_ROW_END16_MAX 65534
#define RG_ROW_END16_WIDE 0xFFFFu
int rg_csr_row_ends16(const void* indptr, int32_t indptr_is_i64, int64_t n_rows, int64_t line_len, int64_t lines_per_plane,
                      uint16_t* row_end16, rg_stream_t stream);
int rg_csr_compact_apply_packed_f32_ex(const void* indptr, int32_t indptr_is_i64, const void* records,
                                       const int64_t* rec_ptr, int32_t rec_order, uint32_t w_base, const int64_t* dict_ptr,
                                       const int32_t* dict, int64_t n_vox, int64_t n_pairs, int64_t line_len,
                                       int64_t lines_per_plane, const float* packed, int32_t n_fields, int32_t stride,
                                       int64_t n_gates, float fill_value, float* out, int32_t window_cap, int32_t tile,
                                       const uint16_t* row_end16, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * K1p  the row-wise kernel in COLUMN MODE, with an optional products epilogue.
 * Replaces, in one pass over the packed records: radar_grid/interpolate.py:69-104 (apply_geometry) / :137-140
 * (apply_geometry_multi) and -- when the caller keeps 2-D products only -- the read-back of the 3-D grid by
 * radar_grid/products.py:462-490 (column_max over a level window) and :361-412 (CAPPI: the two bracketing levels).
 * A workgroup walks the chunks (plane z, line group yg, segment sx) of ONE (yg, sx) through the planes of its level piece,
 * each chunk exactly as rg_csr_compact_apply_packed_f32 (tile = 0) processes it, so lane == row sees its (y, x) column in
 * ascending level order.  Measured: it pays from four field-volumes per pass on (the store it saves is about what walking
 * columns instead of sweeping the grid costs) and always in memory -- no n_fields x 4 x n_vox bytes of grid.
 * Arguments up to fill_value: as rg_csr_compact_apply_packed_f32 (either record order is accepted).
 *   out           [n_fields][n_vox] 3-D grids, or NULL: the grids are not stored (products only);
 *   level_planes  [n_fields][n_keep][ny*nx] or NULL: planes keep_lo .. keep_lo + n_keep - 1 of every field's grid (what a
 *                 CAPPI blends with rg_cappi_lerp_f32, products.py:406-412, or returns as is, :378,386);
 *   col_max / col_arg  [n_fields][ny*nx] or NULL: NaN-ignoring maximum over planes col_lo .. col_hi and the first plane
 *                 attaining it (-1: all NaN) -- the contract of rg_column_reduce_f32(RG_COL_MAX), bit for bit, because lane
 *                 == (y, x) column sees its levels in ascending order;
 *   z_pieces      1 .. planes: a column is cut into this many level ranges, one workgroup each (more workgroups for
 *                 small grids; any value gives the same results).  With col_max and z_pieces > 1 the partial planes live
 *                 in `workspace` (rg_csr_columns_workspace_bytes) and are merged in ascending level order by a second
 *                 small kernel on the same stream;
 *   order         NULL, or a permutation of 0 .. z_pieces * ceil(ny / RG_COMPACT_LINES) * ceil(nx / 64) - 1: workgroup b
 *                 takes item order[b] = piece * columns + (yg * ceil(nx / 64) + c) -- the caller may list the heaviest
 *                 columns first (speed only);
 *   lanes_hint    0, or the diagnostic lane split of the row-wise kernel (1 .. 64 lanes per row, 70 + t).
 * The grids are the same BITS as rg_csr_compact_apply_packed_f32 (tile = 0) for the same lanes_hint (same order of the
 * float32 adds: geometry and field count alone fix it).  At least one of out / level_planes / col_max must be given.
 * ------------------------------------------------------------------------------------------------- */
int64_t rg_csr_columns_workspace_bytes(int64_t lines_per_plane, int64_t line_len, int32_t n_fields, int32_t z_pieces);
int rg_csr_compact_apply_columns_f32(const void* indptr, int32_t indptr_is_i64, const void* records,
                                     const int64_t* rec_ptr, int32_t rec_order, uint32_t w_base, const int64_t* dict_ptr,
                                     const int32_t* dict, int64_t n_vox, int64_t n_pairs, int64_t line_len,
                                     int64_t lines_per_plane, const float* packed, int32_t n_fields, int32_t stride,
                                     int64_t n_gates, float fill_value, float* out, float* level_planes, int32_t keep_lo,
                                     int32_t n_keep, float* col_max, int32_t* col_arg, int32_t col_lo, int32_t col_hi,
                                     int32_t window_cap, int32_t z_pieces, const int32_t* order, void* workspace,
                                     int64_t workspace_bytes, int32_t lanes_hint, rg_stream_t stream);
int rg_csr_compact_apply_columns_f32_ex(const void* indptr, int32_t indptr_is_i64, const void* records,
                                        const int64_t* rec_ptr, int32_t rec_order, uint32_t w_base, const int64_t* dict_ptr,
                                        const int32_t* dict, int64_t n_vox, int64_t n_pairs, int64_t line_len,
                                        int64_t lines_per_plane, const float* packed, int32_t n_fields, int32_t stride,
                                        int64_t n_gates, float fill_value, float* out, float* level_planes, int32_t keep_lo,
                                        int32_t n_keep, float* col_max, int32_t* col_arg, int32_t col_lo, int32_t col_hi,
                                        int32_t window_cap, int32_t z_pieces, const int32_t* order, void* workspace,
                                        int64_t workspace_bytes, int32_t lanes_hint, const uint16_t* row_end16,
                                        rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * K1q  PLANES MODE: the column mode of K1p with a wider products epilogue, for callers that keep 2-D products only.
 * Replaces, in one pass over the packed records, the read-back of the 3-D grid by radar_grid/products.py:462-490
 * (column_max), :493-535 (column_min), :538-580 (column_mean), :361-412 (CAPPI: the two bracketing levels) and :168-314
 * (constant_elevation_ppi: the per-pixel levels, sampled here and combined by rg_elevation_ppi_finish_f32).
 * Arguments up to fill_value and after `req`: as rg_csr_compact_apply_columns_f32; 1-4 fields.  `req` (host memory):
 *   out, level_planes / keep_lo / n_keep, col_max / col_arg, col_lo / col_hi: as rg_csr_compact_apply_columns_f32;
 *   col_min   [n_fields][ny*nx] or NULL: NaN-ignoring minimum over planes col_lo .. col_hi -- the contract of
 *             rg_column_reduce_f32(RG_COL_MIN), bit for bit (np.fmin in ascending level order, all NaN stays NaN);
 *   col_mean  [n_fields][ny*nx] or NULL: NaN-ignoring mean over the same window -- float32 sum of the non-NaN values in
 *             level order and their count, (float)((double)sum / (double)count): rg_column_reduce_f32(RG_COL_MEAN) bit
 *             for bit.  The running sum cannot be split: col_mean needs z_pieces == 1 (RG_EINVAL otherwise);
 *   n_sel     0 .. RG_MAX_SEL_PLANES per-pixel level selections (rg_elevation_ppi_plan_f32): sel_levels[s] is an int32
 *             plane [ny*nx] of lo | hi << 16 or RG_PPI_SEL_NONE; the kernel stores the value of level lo at
 *             sel_samples[f][s][0][pixel] and of level hi at sel_samples[f][s][1][pixel] (pixels with RG_PPI_SEL_NONE
 *             are not written).  sel_samples is [n_fields][n_sel][2][ny*nx]; the grid needs fewer than 65535 planes.
 * At least one of out / level_planes / col_max / col_min / col_mean / a selection must be given.  With z_pieces > 1 the
 * partial maxima (value + arg) and minima (value) live in `workspace` (rg_csr_planes_workspace_bytes) and are merged in
 * ascending level order by a second small kernel.  The grids and every plane are the same BITS as the separate kernels
 * applied to rg_csr_compact_apply_packed_f32's grid (tile = 0, same lanes_hint).
 * ------------------------------------------------------------------------------------------------- */
#define RG_MAX_SEL_PLANES 4
#define RG_PPI_SEL_NONE (-1)

typedef struct rg_plane_request {
  float* out;
  float* level_planes;
  int32_t keep_lo, n_keep;
  float* col_max;
  int32_t* col_arg;
  float* col_min;
  float* col_mean;
  int32_t col_lo, col_hi;
  int32_t n_sel, reserved;
  const int32_t* sel_levels[RG_MAX_SEL_PLANES];
  float* sel_samples;
} rg_plane_request;

/* bytes of `workspace` for z_pieces level pieces: want_max (value + arg) and want_min (value) partial planes */
int64_t rg_csr_planes_workspace_bytes(int64_t lines_per_plane, int64_t line_len, int32_t n_fields, int32_t z_pieces,
                                      int32_t want_max, int32_t want_min);
int rg_csr_compact_apply_planes_f32(const void* indptr, int32_t indptr_is_i64, const void* records,
                                    const int64_t* rec_ptr, int32_t rec_order, uint32_t w_base, const int64_t* dict_ptr,
                                    const int32_t* dict, int64_t n_vox, int64_t n_pairs, int64_t line_len,
                                    int64_t lines_per_plane, const float* packed, int32_t n_fields, int32_t stride,
                                    int64_t n_gates, float fill_value, const rg_plane_request* req, int32_t window_cap,
                                    int32_t z_pieces, const int32_t* order, void* workspace, int64_t workspace_bytes,
                                    int32_t lanes_hint, rg_stream_t stream);
int rg_csr_compact_apply_planes_f32_ex(const void* indptr, int32_t indptr_is_i64, const void* records,
                                       const int64_t* rec_ptr, int32_t rec_order, uint32_t w_base, const int64_t* dict_ptr,
                                       const int32_t* dict, int64_t n_vox, int64_t n_pairs, int64_t line_len,
                                       int64_t lines_per_plane, const float* packed, int32_t n_fields, int32_t stride,
                                       int64_t n_gates, float fill_value, const rg_plane_request* req, int32_t window_cap,
                                       int32_t z_pieces, const int32_t* order, void* workspace, int64_t workspace_bytes,
                                       int32_t lanes_hint, const uint16_t* row_end16, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * a12p / a12f  constant-elevation PPI in two halves around K1q (radar_grid/products.py:168-314).  Scalars, xc / yc and
 * the shape as rg_elevation_ppi_f32.
 * plan:   sel[ny*nx] = lo_s | hi_s << 16 of products.py:280-294 (linear) or ks | ks << 16 of :263-268 (nearest), and
 *         RG_PPI_SEL_NONE where the pixel is NaN whatever the grid holds (linear: target altitude outside [z_min, z_max],
 *         :306-309; nearest: level outside the grid, :266); w_hi[ny*nx] (float64, linear only, else may be NULL) the
 *         upper weight of :284.  nz < 65535.
 * finish: `samples` [2][ny*nx] of one field (K1q's sel_samples[f][s]) -> `out` exactly as rg_elevation_ppi_f32 would
 *         write it from the stored grid: double[ny*nx] w_lo * v_lo + w_hi * v_hi (linear) or float[ny*nx] v_lo (nearest),
 *         NaN where sel is RG_PPI_SEL_NONE.  Both kernels share their per-pixel code with rg_elevation_ppi_f32.
 * ------------------------------------------------------------------------------------------------- */
int rg_elevation_ppi_plan_f32(const float* xc, const float* yc, int32_t nz, int32_t ny, int32_t nx, double cos_clamped,
                              double sin_elev, double tan_elev, double ke_re, double ke_re_sq, double z_min, double z_max,
                              double z_step, int32_t earth_curvature, int32_t linear, int32_t* sel, double* w_hi,
                              rg_stream_t stream);
int rg_elevation_ppi_finish_f32(const int32_t* sel, const double* w_hi, const float* samples, int64_t n_xy, int32_t linear,
                                void* out, rg_stream_t stream);

/* number of chunks of a grid of n_rows rows (negative rg_status when the sizes do not factor) */
int64_t rg_csr_compact_chunks(int64_t n_rows, int64_t line_len, int64_t lines_per_plane);

/* Building the compact copy from a standard CSR, or from a slab of whole planes of it: pass indptr + first row of the
 * slab, n_rows of the slab, and gate_idx / local_idx pointers such that element p is ABSOLUTE pair p (the row pointers
 * hold absolute pair positions).  rg_csr_compact_count: chunk_counts[c] = dictionary entries of chunk c (header
 * included for a split chunk; >= 0x40000000 = a single segment references more than 65536 gates: not compactable),
 * chunk_rounds[c] = hashing rounds the chunk needed and its split flag (opaque, handed to the fill pass).  The caller turns the counts into dict_ptr (rg_scan_counts_i64, chunk_counts needs one
 * spare entry) and calls rg_csr_compact_fill, which writes dict[dict_ptr[c] ..] and local_idx[p] for every pair.
 * Dictionary order is unspecified.  *error_flag (device int32, zeroed by the caller) becomes non-zero when the fill
 * pass meets inputs that differ from what the count pass saw (gate_idx modified in between, wrong chunk_rounds):
 * every table walk is bounded, so such a mismatch is reported instead of hanging the GPU. */
int rg_csr_compact_count(const void* indptr, int32_t indptr_is_i64, const int32_t* gate_idx, int64_t n_rows,
                         int64_t line_len, int64_t lines_per_plane, int32_t* chunk_counts, uint8_t* chunk_rounds,
                         rg_stream_t stream);
int rg_csr_compact_fill(const void* indptr, int32_t indptr_is_i64, const int32_t* gate_idx, int64_t n_rows,
                        int64_t line_len, int64_t lines_per_plane, const int64_t* dict_ptr,
                        const uint8_t* chunk_rounds, int32_t* dict, uint16_t* local_idx, int32_t* error_flag,
                        rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Georeferencing: a radar's gates into the plane of a shared grid, and a grid's nodes to longitude / latitude.  (No
 * reference counterpart in radar_grid; the projection is PyART's `pyart_aeqd` -- azimuthal equidistant on a SPHERE of
 * radius 6370997 m -- restated from its formulas.  PyART is not in the tree: parity with it is unpinned.)
 *
 * rg_georef is a HOST struct, filled once in float64 (radar_processor_amd/georef.py: make_georef) and passed by value to
 * the kernels, which evaluate no trigonometry of its constants.  Angles in radians.
 *   inverse, plane (x, y) about (lon_from, lat_from) -> (lon, lat):
 *     rho = hypot(x, y); c = rho / radius; (sc, cc) = sincos(c)
 *     lat = asin(clamp(cc * sin_lat_from + y * sc * cos_lat_from / rho, -1, 1))
 *     lon = lon_from + atan2(x * sc, rho * cos_lat_from * cc - y * sin_lat_from * sc)
 *     rho == 0: the centre (lon_from, lat_from).
 *   forward, (lon, lat) -> plane about (lon_to, lat_to):
 *     d = lon - lon_to; (sp, cp) = sincos(lat); (sd, cd) = sincos(d)
 *     a = cp * sd;  b = cos_lat_to * sp - sin_lat_to * cp * cd;  q = sin_lat_to * sp + cos_lat_to * cp * cd
 *     s = hypot(a, b); k = atan2(s, q) / s (1 where s == 0);  X = radius * k * a;  Y = radius * k * b
 * Every step is float64, unfused, in the order written; results are rounded once.
 * ------------------------------------------------------------------------------------------------- */
typedef struct rg_georef {
  double radius;                               /* of the sphere, metres: finite, > 0 */
  double lon_from, lat_from;                   /* centre of the plane the inputs lie in */
  double sin_lat_from, cos_lat_from;
  double lon_to, lat_to;                       /* centre of the plane of the outputs (rg_gates_to_frame_f32 only) */
  double sin_lat_to, cos_lat_to;
  double ox, oy;                               /* forward(lon_from, lat_from): the `from` centre in the `to` plane */
  int32_t same_centre;                         /* 1: both centres are the same point (ox = oy = 0): copy, do not project */
  int32_t reserved;
} rg_georef;

/* x_out[i] = (float)(X - ox), y_out[i] = (float)(Y - oy) with (X, Y) = forward(inverse(x[i], y[i])): gate i of a radar at
 * the `from` centre, relative to its antenna's position (ox, oy) in the plane about the `to` centre.  A gate whose x or y
 * is not finite gives NaN in both outputs; rho == 0 gives (0, 0).  same_centre: x and y are copied bit for bit, whatever
 * they hold.  One thread per gate.  An input may BE an output (equal pointers: in place); arrays that overlap in any other
 * way are refused (RG_EINVAL), as are null pointers, n < 0 and a radius or any other member that is not finite.  n == 0
 * returns RG_OK without a launch. */
int rg_gates_to_frame_f32(const float* x, const float* y, int64_t n, const rg_georef* radar_to_grid, float* x_out,
                          float* y_out, rg_stream_t stream);
/* lon[iy*nx + ix], lat[iy*nx + ix] (float64 degrees, lon in [-180, 180)) = inverse(xc[ix], yc[iy]) about the `from` centre
 * of `grid`: the geographic position of every node of a grid's float32 coordinate tables.  One thread per node.  A table
 * entry that is not finite gives NaN in both planes.  Refusals as above (every member of `grid` must be finite); ny == 0 or
 * nx == 0 returns RG_OK without a launch. */
int rg_frame_to_lonlat_f64(const float* xc, const float* yc, int32_t ny, int32_t nx, const rg_georef* grid, double* lon,
                           double* lat, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Onto a web map: a product plane (or its RGBA image) resampled north-up into a Web Mercator (EPSG:3857) raster, and the
 * overview pyramid of such an image.  (Reference: radar_processor/processor.py:229-303 shells out to gdalwarp and :306-420
 * lets rasterio build the overviews; radar_grid/geotiff.py:238-291 does not resample at all.)
 *
 * Two HOST structs, passed by value to the kernels like rg_georef:
 *   rg_mercator_raster  the destination.  The pixel is square; row 0 is the NORTHERNMOST row; the centre of pixel (r, c) is
 *                       X = x_min + (c + 0.5) * pixel,  Y = y_max - (r + 0.5) * pixel   (EPSG:3857 metres).
 *   rg_warp_source      the float64 lattice of a plane [ny, nx]: node (iy, ix) lies at (x_lo + ix * step_x, y_lo + iy * step_y)
 *                       of the grid's AEQD plane, step = (hi - lo) / (n - 1) > 0; row iy grows NORTHWARDS, as in every grid
 *                       here.  The gridders' float32 node tables (np.linspace(..., dtype='float32')) differ from this lattice
 *                       by at most half a float32 ulp of the limits -- millimetres for any grid a radar fills.
 * The map of one destination pixel, float64, unfused, in this order:
 *     a = 6378137 (the EPSG:3857 sphere);  t = Y / a;  sp = tanh(t);  cp = 1 / cosh(t);  lam = X / a
 *     (sd, cd) = sincos(lam - lon_to)
 *     (Xg, Yg) = the AEQD forward map above about (lon_to, lat_to) of the rg_georef, fed sp, cp, sd and cd;  c = atan2(s, q)
 *     c >= pi/2 - 0.1  ->  the pixel is fill (georef.MAX_ANGULAR_DISTANCE: without it the far hemisphere folds back into
 *                          the grid's plane)
 *     fx = (Xg - x_lo) / step_x;  fy = (Yg - y_lo) / step_y          (plane coordinates in nodes)
 * sp and cp are the sine and cosine of the latitude whose Mercator ordinate is Y, so no latitude is ever formed.  The map is
 * periodic in lam: x_min may lie beyond +-pi * a (a grid across the antimeridian gets one connected raster).
 * Longitude and latitude are carried UNCHANGED from the 6370997 m sphere of the grid to the 6378137 m sphere of EPSG:3857 --
 * what a PROJ pipeline with no datum shift does.  Parity with gdalwarp is UNPINNED: GDAL, pyproj and rasterio are not in the
 * tree; the tests pin the map against a 40-digit evaluation of these formulas.
 * ------------------------------------------------------------------------------------------------- */
typedef struct rg_mercator_raster {
  double x_min, y_max;                         /* outer edge of the west-most column / of the north-most row, metres: finite */
  double pixel;                                /* side of a pixel, metres: finite, > 0 */
  int32_t width, height;                       /* >= 0 */
} rg_mercator_raster;

typedef struct rg_warp_source {
  double x_lo, y_lo;                           /* node (0, 0) in the grid's plane, metres: finite */
  double step_x, step_y;                       /* node spacing, metres: finite, > 0 */
  int32_t ny, nx;                              /* >= 2 */
} rg_warp_source;

/* out[p][r][c] for p < n_planes: plane p of src ([n_planes, ny, nx] float32) sampled at (fx, fy) of pixel (r, c); one
 * coordinate evaluation serves all planes of a pixel.  out is [n_planes, height, width].
 *   method 0, nearest:  ix = floor(fx + 0.5), iy = floor(fy + 0.5); outside 0 <= ix < nx, 0 <= iy < ny the pixel is `fill`,
 *     inside it the source value is copied bit for bit (NaN and inf included).
 *   method 1, bilinear: x0 = floor(fx), tx = fx - x0, likewise y.  The taps (y0,x0), (y0,x0+1), (y0+1,x0), (y0+1,x0+1), in
 *     that order, carry the float64 weights (1-ty)(1-tx), (1-ty)tx, ty(1-tx), ty*tx.  A tap outside the plane, or one that
 *     is NaN, is missing; wsum and vsum (weight * value) are summed in float64 over the taps present, in that order;
 *     out = (float)(vsum / wsum) if wsum >= 0.5, else `fill` -- an echo's edge stays where nearest keeps it.
 * Refused with RG_EINVAL before any launch: null pointers, n_planes < 1, a struct member that is not finite or not positive
 * where it must be (a negative width or height included), ny or nx below 2, an unknown method, out overlapping src.
 * width == 0 or height == 0 returns RG_OK without a launch.  Rasters of more than 2^31 pixels take several launches. */
int rg_warp_mercator_f32(const float* src, int32_t n_planes, const rg_warp_source* source, const rg_georef* grid,
                         const rg_mercator_raster* raster, int32_t method, float fill, float* out, rg_stream_t stream);
/* The same map for an RGBA image: src [ny, nx, 4] uint8 -> out [height, width, 4] uint8 (both 4-byte aligned, RG_EALIGN
 * otherwise), nearest only, one 32-bit load and store per pixel.  A sample outside the plane, or beyond the angular limit,
 * gives 0, 0, 0, 0.  Refusals as above. */
int rg_warp_mercator_rgba8(const uint8_t* src, const rg_warp_source* source, const rg_georef* grid,
                           const rg_mercator_raster* raster, uint8_t* out, rg_stream_t stream);
/* One overview level of src [n_planes, h, w] float32: out is [n_planes, ceil(h / factor), ceil(w / factor)].  Every level
 * is computed from the base image, never from another level.
 *   method 0, nearest: out[r][c] = src[min(r * f + f / 2, h - 1)][min(c * f + f / 2, w - 1)], bit for bit.
 *   method 1, average: the mean of the FINITE values of the block [r * f, min((r + 1) * f, h)) x [c * f, min((c + 1) * f, w)),
 *     accumulated in float64 in row-major order and rounded once to float32; a block with no finite value gives NaN.
 * 2 <= factor <= 64.  Refused with RG_EINVAL: null pointers, n_planes < 1, h or w negative, a factor out of range, an unknown
 * method, out overlapping src.  h == 0 or w == 0 returns RG_OK without a launch. */
int rg_overview_f32(const float* src, int32_t n_planes, int32_t h, int32_t w, int32_t factor, int32_t method, float* out,
                    rg_stream_t stream);
/* The nearest rule of rg_overview_f32 for an RGBA image [h, w, 4] uint8 (4-byte aligned): one 32-bit load and store. */
int rg_overview_rgba8(const uint8_t* src, int32_t h, int32_t w, int32_t factor, uint8_t* out, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Connected echo regions: labelling, the per-cell table and despeckling.  (No reference counterpart in radar_grid; the
 * numbering is scipy.ndimage.label's, the sweep use with wrap_rows is PyART's despeckle_field.  Neither is in the tree: the
 * tests pin the contract against a flood fill, tests/components_oracle.py.)
 *
 * Input: n_planes independent float32 planes [h][w], row-major, n_planes * h * w < 2^31 (RG_EINVAL otherwise).
 *   foreground   v >= lo && v <= hi in float32, and mask (optional uint8 of the planes' shape) zero at the pixel.  lo is
 *                inclusive; hi may be +inf, and then +inf is foreground; NaN never is (both comparisons fail).
 *   neighbours   connectivity 4: (y +- 1, x), (y, x +- 1); 8: the diagonals too.  wrap_rows != 0: row 0 and row h - 1 of the
 *                SAME plane are neighbours (with 8, their diagonals included) -- the azimuth wrap of a sweep [n_rays, n_gates].
 *                Planes never connect to each other.
 * How it runs: one workgroup labels a tile of RG_CC_TILE_H x RG_CC_TILE_W pixels with a union-find in LDS; a second launch
 * unites the pixel pairs across tile borders (the corner diagonals and the wrap seam included) with agent-scope atomic
 * minima; further launches resolve every pixel to its root, rank the roots with a scan and write the ids.  The larger root is
 * always linked under the smaller, so a cell's root is its smallest flat index = its first pixel in raster order, and ranking
 * the roots in index order IS the raster-order numbering.  No workgroup ever waits for another.
 * ------------------------------------------------------------------------------------------------- */
#define RG_CC_TILE_H 32
#define RG_CC_TILE_W 64

/* bytes of `workspace` rg_label_components_f32 needs for these sizes (a multiple of 16), or RG_EINVAL (as int64) */
int64_t rg_components_workspace_bytes(int32_t n_planes, int32_t h, int32_t w);
/* labels: int32 [n_planes][h][w], 0 = background, the cells of plane p numbered 1 .. (cells of p) in raster order of each
 * cell's FIRST pixel.  cell_ptr: int32 [n_planes + 1] on the device, the exclusive running count of cells: cell k of plane p
 * is row cell_ptr[p] + k - 1 of any per-cell array, cell_ptr[n_planes] the number of cells.  mask may be NULL.  workspace:
 * 4-byte aligned, at least rg_components_workspace_bytes (RG_EWORKSPACE otherwise), contents undefined before and after.
 * Refused with RG_EINVAL: null pointers, n_planes < 1, h or w negative, the size limit, lo or hi NaN, connectivity not 4 or 8,
 * labels overlapping src.  h == 0 or w == 0 zeroes cell_ptr and returns. */
int rg_label_components_f32(const float* src, const uint8_t* mask, int32_t n_planes, int32_t h, int32_t w, float lo, float hi,
                            int32_t connectivity, int32_t wrap_rows, int32_t* labels, int32_t* cell_ptr, void* workspace,
                            int64_t workspace_bytes, rg_stream_t stream);
/* The table of the cells of `labels` / `cell_ptr` (as written by rg_label_components_f32) over the values of `src`: per-cell
 * arrays of n_cells rows (n_cells = cell_ptr[n_planes], read by the caller); any output pointer may be NULL.
 *   area     int32      pixels of the cell
 *   bbox     int32 [4]  y_min, y_max, x_min, x_max
 *   sum_yx   int64 [2]  sum of y, sum of x over the cell's pixels (integers: sum / area is the exact centroid)
 *   vmax     float32    the largest value;  argmax int32: its flat index y * w + x within the plane, the smallest index among
 *                       ties.  Order: the IEEE total order of the non-NaN values (-0 below +0); a NaN pixel takes no part, a
 *                       cell with no other value gets vmax = NaN, argmax = -1.  argmax needs vmax (RG_EINVAL without it): the
 *                       maximum is formed in vmax's own words as an order-preserving 32-bit key with atomic maxima, then the
 *                       pixels that hold it race for the smallest index with atomic minima -- two order-independent steps.
 *   vsum     float64    sum of the cell's values (float64 atomic adds of per-run partial sums: the one output that depends
 *                       on the order of arrival, within n * 2^-53 * sum|v|)
 * Every other output is bit-reproducible.  Indices are RAW: under wrap_rows a cell across the seam is NOT unwrapped -- its
 * bbox spans 0 .. h - 1 and its centroid lies between its two parts.  Equal-label runs of a wavefront's 64 consecutive pixels
 * are combined first and issue ONE atomic per run and output, so a plane that is one cell is not one atomic per pixel.
 * n_cells == 0 returns RG_OK without a launch; a label that points beyond n_cells is ignored. */
int rg_component_stats_f32(const float* src, const int32_t* labels, const int32_t* cell_ptr, int32_t n_planes, int32_t h,
                           int32_t w, int32_t n_cells, int32_t* area, int32_t* bbox, int64_t* sum_yx, float* vmax,
                           int32_t* argmax, double* vsum, rg_stream_t stream);
/* out[p][i] = fill where labels[p][i] > 0 and area[cell_ptr[p] + labels[p][i] - 1] < min_size, else src[p][i] bit for bit
 * (background pixels are never touched).  out_mask (optional uint8 of the planes' shape): 1 where the pixel was removed, else
 * 0 -- the kind of mask the gridders' `masks` arguments take.  src == out is allowed (in place); any other overlap is not
 * checked.  min_size < 1 is RG_EINVAL. */
int rg_despeckle_select_f32(const float* src, const int32_t* labels, const int32_t* cell_ptr, const int32_t* area,
                            int32_t n_planes, int32_t h, int32_t w, int32_t min_size, float fill, float* out,
                            uint8_t* out_mask, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Echo motion and nowcasts: the motion field between two successive product planes by block matching, and the plane
 * extrapolated along it (semi-Lagrangian advection).  (No reference counterpart in radar_grid; the tests pin the three
 * kernels to the NumPy restatement of exactly these formulas, tests/motion_oracle.py.)  rg_motion_quantize_f32,
 * rg_block_match_u8 and rg_advect_f32 were ADDED; no signature changed, RG_VERSION stays 104.
 *
 * SIGN AND UNITS: echo at pixel p of `prev` is found at p + motion in `next`; motion is (dy, dx) in pixels per interval
 * between the two planes.  Row index grows NORTHWARDS, as in every grid here, so dy > 0 is northward and dx > 0 eastward.
 * Planes are [n][h][w], row-major, pitch w, no padding, n * h * w < 2^31 (RG_EINVAL otherwise).
 * ------------------------------------------------------------------------------------------------- */
#define RG_MOTION_MAX_BLOCK 64
#define RG_MOTION_MAX_SEARCH 32
#define RG_MAX_LEADS 16

/* Planes to 8-bit levels: src float32 [n][h][w], mask (optional, may be NULL) uint8 of the same shape, out uint8 of the
 * same shape.  inv_step is float32(254 / (hi - lo)), formed by the host from doubles.  Per pixel, in float32:
 *     q = 0                                      where mask != 0 or `v >= lo` is false (NaN and -inf included)
 *     t = (v - lo) * inv_step                    two float32 operations, unfused
 *     q = 1 + (t >= 254 ? 254 : (int)t)          otherwise
 * Level 0 is "no echo", 1 .. 255 are echo; +inf and everything above hi give 255.
 * RG_EINVAL: a null src or out, n < 1, h or w negative, the size limit, lo or inv_step not finite, inv_step <= 0.
 * h == 0 or w == 0 returns RG_OK without a launch. */
int rg_motion_quantize_f32(const float* src, const uint8_t* mask, int32_t n, int32_t h, int32_t w, float lo, float inv_step,
                           uint8_t* out, rg_stream_t stream);

/* One motion vector per block of `prev`, searched in `next` (both uint8 [n][h][w] as written by rg_motion_quantize_f32; they
 * may be the views q[:-1] and q[1:] of one stack of n + 1 planes).
 *   block B      4 <= B <= RG_MOTION_MAX_BLOCK, B % 4 == 0;  N = B * B
 *   stride S     >= 1;  nby = (h - B) / S + 1, nbx = (w - B) / S + 1;  h < B or w < B is RG_EINVAL
 *   search R     0 <= R <= RG_MOTION_MAX_SEARCH
 *   min_echo     1 <= min_echo <= N
 * Block (by, bx) is prev[by*S : by*S + B, bx*S : bx*S + B].  With a the block's levels and b those of a shifted window of
 * `next`, all sums exact integers (Sa = sum a, Saa = sum a*a, Sb, Sbb, Sab likewise; Sab <= 4096 * 255^2 < 2^31):
 *   valid block    at least min_echo non-zero levels, and va = N*Saa - Sa*Sa > 0
 *   candidates     (dy, dx) in [-R, R]^2 whose window next[by*S + dy : .. + B, bx*S + dx : .. + B] lies wholly inside the
 *                  plane and has vb = N*Sbb - Sb*Sb > 0 ("qualified")
 *   score          s = (double)(N*Sab - Sa*Sb) / sqrt((double)va * (double)vb)     the numerator an int64; the float64
 *                  product, square root and quotient are each rounded once, so s has the bits NumPy computes
 *   winner         the largest s; ties go to the smallest dy*dy + dx*dx, then the smallest dy, then the smallest dx
 *   sub-pixel      per axis, float64: m and p the scores of the winner's two neighbours on that axis; if both are qualified
 *                  candidates inside [-R, R] and den = m - 2*s0 + p < 0 then off = clamp(0.5 * (m - p) / den, -0.5, 0.5),
 *                  else off = 0
 * Outputs per block:  disp int16 [n][nby][nbx][2] = (dy, dx);  motion float32 [n][nby][nbx][2] = ((float)(dy + off_y),
 * (float)(dx + off_x));  score float32 [n][nby][nbx] = (float)s0.  An invalid block, or one with no qualified candidate,
 * gives disp = (0, 0) and NaN in motion and score.
 * How it runs: one workgroup per block; the block and its (B + 2R)^2 window are staged in LDS (window bytes outside the
 * plane as 0: no qualified candidate reads them); Sab, Sb and Sbb come from the packed 8-bit dot product, a dx that is no
 * multiple of 4 by byte-aligning two LDS dwords; the scores of all (2R + 1)^2 candidates stay in LDS for the arg-max over the
 * full tie key and for the parabola.  No byte outside [0, n*h*w) of either input is read (rows are not 4-byte aligned when
 * w % 4 != 0: staging loads bytes).  No atomics, no workgroup waits for another, every output is bit-reproducible.
 * RG_EINVAL before any launch: null pointers, n < 1, h or w negative, the size limit, a parameter outside its range. */
int rg_block_match_u8(const uint8_t* prev, const uint8_t* next, int32_t n, int32_t h, int32_t w, int32_t block, int32_t stride,
                      int32_t search, int32_t min_echo, int16_t* disp, float* motion, float* score, rg_stream_t stream);

/* The node lattice of a motion field [ny][nx][2], components (v, u) = (dy, dx): node (j, i) lies at pixel
 * (origin_y + j * step_y, origin_x + i * step_x).  For a block-match lattice origin = (B - 1) / 2.0 and step = S; a dense
 * per-pixel field is 0, 0, 1, 1.  A HOST struct, passed by value. */
typedef struct rg_motion_lattice {
  double origin_y, origin_x;                   /* pixel coordinates of node (0, 0): finite */
  double step_y, step_x;                       /* node spacing in pixels: finite, > 0 */
  int32_t ny, nx;                              /* >= 1 */
} rg_motion_lattice;

/* Semi-Lagrangian extrapolation: out[l][p][y][x] = plane p of src ([n_planes][h][w] float32) sampled where the echo that
 * reaches pixel (y, x) after leads_host[l] intervals sits now.  One displacement per pixel and lead serves all planes.
 * `motion` float32 [ny][nx][2] on the device, ALL FINITE (the caller's duty; a NaN vector makes the pixels it reaches
 * `fill`, never a fault).  Everything up to the sample is float64, unfused, in this order.
 *   motion at a point (py, px):   ly = clamp((py - origin_y) / step_y, 0, ny - 1);  j0 = min(floor(ly), max(ny - 2, 0));
 *       j1 = min(j0 + 1, ny - 1);  ty = ly - j0;  likewise lx, i0, i1, tx;  per component
 *       V = (V[j0,i0]*(1-tx) + V[j0,i1]*tx)*(1-ty) + (V[j1,i0]*(1-tx) + V[j1,i1]*tx)*ty
 *       -- constant extrapolation beyond the outermost nodes
 *   displacement:   d = (0, 0);  `substeps` times:  d = d + (lead / substeps) * V(p - d);  the source position is p - d
 *   sampling (fy, fx) = p - d:   exactly the two rules of rg_warp_mercator_f32 (the kernels share csrc/rg_sample.hpp):
 *       method 0, nearest: iy = floor(fy + 0.5), ix = floor(fx + 0.5), the value copied bit for bit, `fill` outside the plane;
 *       method 1, bilinear: the four taps in that order, NaN and outside taps missing, wsum and vsum in float64,
 *       out = (float)(vsum / wsum) if wsum >= 0.5, else `fill`.
 * leads_host: n_leads <= RG_MAX_LEADS finite doubles in units of the interval, read on the host and passed by value.
 * 1 <= substeps <= 16.  Lead 0 returns src bit for bit under nearest.
 * RG_EINVAL before any launch: null pointers, n_planes < 1, h or w negative, the size limit, n_leads outside
 * 0 .. RG_MAX_LEADS, a lead or a lattice member that is not finite, a step <= 0, ny or nx < 1, substeps out of range, an
 * unknown method, out overlapping src.  h == 0, w == 0 or n_leads == 0 returns RG_OK without a launch. */
int rg_advect_f32(const float* src, int32_t n_planes, int32_t h, int32_t w, const float* motion, rg_motion_lattice lattice,
                  const double* leads_host, int32_t n_leads, int32_t substeps, int32_t method, float fill, float* out,
                  rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Cell overlap and tracking: which cell of one labelling is which cell of another -- the contingency table of two label
 * planes -- and the map from a label plane to any per-cell integer (a track id).  (No reference counterpart in radar_grid;
 * every output is an integer and the tests pin them to np.unique, tests/tracking_oracle.py.)  rg_cell_overlap_workspace_bytes,
 * rg_cell_overlap_i32 and rg_relabel_cells_i32 were ADDED; no signature changed, RG_VERSION stays 104.
 *
 * labels_* int32 [n_planes][h][w] and cell_ptr_* int32 [n_planes + 1] are what rg_label_components_f32 writes;
 * n_planes * h * w < 2^31 (RG_EINVAL otherwise).  Plane p of `prev` is paired with plane p of `next`; the two may be the views
 * L[:-1] and L[1:] of one stack, each with its own cell_ptr.
 *   pairs      a pixel with labels a > 0 and b > 0 belongs to the pair (row_prev, row_next) = (cell_ptr_prev[p] + a - 1,
 *              cell_ptr_next[p] + b - 1): the rows of the two cell tables.  A pixel with a <= 0 or b <= 0 takes no part, nor
 *              does a label above its plane's cell count cell_ptr[p + 1] - cell_ptr[p].
 *   table      open addressing in `workspace`, capacity C = the smallest power of two >= max(2 * max_pairs, 64): 64-bit keys
 *              (uint64)row_prev << 32 | row_next, all ones = empty (unreachable: rows stay below 2^31), and 32-bit counts.
 * How it runs: the entry point clears the table and totals on `stream` (hipMemsetAsync).  One thread per pixel, a wavefront
 * covering 64 consecutive flat indices; runs of lanes with an equal pair are found with one ballot (csrc/rg_lane_runs.hpp, shared
 * with the cell table) and only a run's last lane inserts, with the run's length.  It claims a slot with an agent-scope relaxed
 * 64-bit compare-and-swap and adds the length with a relaxed 32-bit atomic add; probing is linear, visits at most C slots, then
 * bumps totals[1] and gives up.  A compare-and-swap finds the slot empty and claims it, finds the key equal, or moves on: no
 * thread waits for another, no loop is unbounded.  A second launch compacts the occupied slots into the outputs behind an atomic
 * cursor (totals[0], one atomic per wavefront).  The hash (splitmix64's finaliser) shows in nothing but the order of the entries.
 * ------------------------------------------------------------------------------------------------- */

/* bytes of `workspace` rg_cell_overlap_i32 needs for max_pairs (12 * C, a multiple of 16), or RG_EINVAL (as int64) for
 * max_pairs < 1 or max_pairs >= 2^30 */
int64_t rg_cell_overlap_workspace_bytes(int64_t max_pairs);
/* pair_rows int32 [max_pairs][2] = (row_prev, row_next) and pair_count int32 [max_pairs] = the pixels the two cells share: one
 * entry per distinct pair, in unspecified order; only min(totals[0], max_pairs) entries are written.  totals int32 [2]:
 *   totals[0]   the number of distinct pairs held in the table; it may exceed max_pairs (up to C)
 *   totals[1]   the number of insertions that found the table full and were dropped
 * The result is COMPLETE iff totals[0] <= max_pairs && totals[1] == 0; then the SET of (row_prev, row_next, count) triples is
 * bit-reproducible.  An incomplete result is still RG_OK, and every entry written is a true pair whose count holds the
 * insertions that reached the table (the full count while totals[1] == 0).  workspace: 8-byte aligned, at least
 * rg_cell_overlap_workspace_bytes(max_pairs) (RG_EWORKSPACE otherwise), contents undefined before and after.
 * RG_EINVAL before any launch: null pointers, n_planes < 1, h or w negative, the size limit, max_pairs < 1 or >= 2^30, an output
 * or the workspace overlapping an input.  h == 0 or w == 0 zeroes totals and returns. */
int rg_cell_overlap_i32(const int32_t* labels_prev, const int32_t* cell_ptr_prev, const int32_t* labels_next,
                        const int32_t* cell_ptr_next, int32_t n_planes, int32_t h, int32_t w, int64_t max_pairs,
                        int32_t* pair_rows, int32_t* pair_count, int32_t* totals, void* workspace, int64_t workspace_bytes,
                        rg_stream_t stream);
/* out[p][i] = lut[cell_ptr[p] + labels[p][i] - 1] where 0 < labels[p][i] <= cell_ptr[p + 1] - cell_ptr[p] and that row lies
 * below n_cells, else 0.  lut: int32 [n_cells], any per-cell integer -- track ids give the track plane for display.
 * out == labels is allowed (in place); any other overlap of out with an input is RG_EINVAL.  n_cells == 0 writes zeros (lut may
 * then be NULL).  RG_EINVAL: null pointers, n_planes < 1, h or w negative, the size limit, n_cells < 0.  h == 0 or w == 0
 * returns RG_OK without a launch. */
int rg_relabel_cells_i32(const int32_t* labels, const int32_t* cell_ptr, int32_t n_planes, int32_t h, int32_t w,
                         const int32_t* lut, int32_t n_cells, int32_t* out, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Rain rate and accumulation: reflectivity planes as rain rates (Z = a R^b), and the rainfall depth of the interval between
 * two rate planes summed ALONG the echo's motion, so that a cell moving several pixels per scan leaves a swath and not a row
 * of separate blobs.  (No reference counterpart in radar_grid; the tests pin both kernels to the NumPy restatement of exactly
 * these formulas, tests/accumulation_oracle.py.)  rg_rain_rate_f32 and rg_accumulate_advected_f32 were ADDED; no signature
 * changed, RG_VERSION stays 104.
 *
 * Planes are [n][h][w], row-major, pitch w, no padding, n * h * w < 2^31 (RG_EINVAL otherwise).  Motion, its sign, its units
 * and rg_motion_lattice are those of "Echo motion and nowcasts".  A rate plane has three kinds of pixel: NaN = no coverage
 * (never measured), 0 = covered and dry, > 0 = rain in mm/h.
 * ------------------------------------------------------------------------------------------------- */
#define RG_MAX_ACC_STEPS 64

/* dBZ to mm/h under Z = a R^b: src float32 [n][h][w] in dBZ, mask (optional, may be NULL) uint8 of the same shape, out float32
 * of the same shape.  The host passes the doubles p = ln(10) / (10 b) and q = ln(a) / b, so that R = exp(dBZ * p - q).
 * Per pixel, v = src:
 *     out = quiet NaN 0x7FC00000                 where mask != 0 or v is NaN                      "no coverage"
 *     out = 0.0f                                 where `v >= min_dbz` is false (-inf included)    "covered, dry"
 *     c = min((double)v, max_dbz);  out = (float)exp(c * p - q)       otherwise: one float64 multiply, one subtract and one
 *                                                exp, unfused; +inf and everything above max_dbz give the rate at max_dbz
 * The multiply and the subtract are rounded once each, so the argument of exp has NumPy's bits; the device's exp and the
 * host's each lie within 1 ulp(float64) of the true value, so the float32 result is the host's or its float32 neighbour.
 * RG_EINVAL: a null src or out, n < 1, h or w negative, the size limit, p not finite or not positive, q, min_dbz or max_dbz not
 * finite, max_dbz < min_dbz.  h == 0 or w == 0 returns RG_OK without a launch. */
int rg_rain_rate_f32(const float* src, const uint8_t* mask, int32_t n, int32_t h, int32_t w, double p, double q, double min_dbz,
                     double max_dbz, float* out, rg_stream_t stream);

/* Advection-corrected accumulation over one interval: rate_prev and rate_next float32 [n_planes][h][w] are the rates at the two
 * ends of an interval of `hours` (finite, > 0); out float32 [n_planes][h][w] is the depth (rate unit * hours: mm for mm/h);
 * out_steps (optional, may be NULL) uint8 [n_planes][h][w] is the number of sub-instants that contributed.  rate_prev and
 * rate_next may be the same plane.  `motion` float32 [ny][nx][2] on the device and `lattice` are exactly those of rg_advect_f32:
 * the motion from prev to next, ALL FINITE (the caller's duty; a NaN vector makes the samples it reaches missing, never a fault
 * -- the same clamp before any index).
 *   pos(p, lead)   the source position of rg_advect_f32 for pixel p: d = (0, 0);  `substeps` times
 *                  d = d + (lead / substeps) * V(p - d);  pos = p - d, with the same lattice interpolant V, all float64, in that
 *                  order.  A negative lead moves the sample FORWARD along the motion.
 *   for k = 0 .. n_steps - 1, in this order:
 *       s = ((double)k + 0.5) / (double)n_steps
 *       a = the sample of rate_prev at pos(p, s);   b = the sample of rate_next at pos(p, s - 1.0)
 *           -- by `method` (0 nearest, 1 bilinear), the two rules of rg_advect_f32 with NaN as the fill: each sample is bit for
 *           bit the float32 rg_advect_f32 writes for that lead.  A sample is MISSING when it is NaN: a position outside the
 *           plane, a NaN source pixel, bilinear wsum < 0.5
 *       both present:   r = (1.0 - s) * (double)a + s * (double)b
 *       one present:    r = (double) that sample
 *       none present:   the step is missing
 *       a present step: total = total + r;  n = n + 1
 *   out = n >= min_steps ? (float)(hours * (total / (double)n)) : fill;      out_steps = n
 * All float64, unfused, each operation rounded once.  One set of positions serves all planes.  With zero motion this is the
 * midpoint rule of the linear blend in time -- the trapezoid rule's value; with n_steps = 1 and prev == next it is hours * rate.
 *   1 <= n_steps <= RG_MAX_ACC_STEPS;  1 <= substeps <= 16;  1 <= min_steps <= n_steps
 * How it runs: one thread per pixel, a workgroup per tile of 8 x 32 pixels; the loop over k and the totals of up to four planes
 * stay in registers (more planes: further workgroups, and beyond 65535 groups of four further launches); V(p), the first step of every displacement of a pixel, is evaluated once,
 * so substeps == 1 reads the lattice once per pixel for all 2 * n_steps positions; s, s / substeps and (s - 1) / substeps are the
 * same for every pixel and are formed by the entry point on the host, in float64 as written above, and passed by value.  Every
 * index is formed after its inside test.  No atomics, no LDS, no workgroup waits for another, no loop beyond n_steps * substeps; every output is
 * bit-reproducible.
 * RG_EINVAL before any launch: a null rate_prev, rate_next, motion or out, n_planes < 1, h or w negative, the size limit, a
 * lattice member that is not finite, a step <= 0, ny or nx < 1, hours not finite or <= 0, n_steps, substeps or min_steps out of
 * range, an unknown method, out or out_steps overlapping an input or each other.  h == 0 or w == 0 returns RG_OK without a
 * launch. */
int rg_accumulate_advected_f32(const float* rate_prev, const float* rate_next, int32_t n_planes, int32_t h, int32_t w,
                               const float* motion, rg_motion_lattice lattice, double hours, int32_t n_steps, int32_t substeps,
                               int32_t method, int32_t min_steps, float fill, float* out, uint8_t* out_steps, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Nowcast verification: how good a forecast plane is against the observation it was made for -- categorical counts at
 * thresholds, the three sums of the fractions skill score (FSS) over a ladder of neighbourhood sizes, and the neighbourhood
 * exceedance fraction as a product.  (No reference counterpart in radar_grid.  Every sum is an integer and every atomic an
 * integer add, so every output is bit-reproducible; the tests hold them EQUAL to the NumPy restatement of exactly these
 * definitions, tests/verification_oracle.py.  The window is scipy.ndimage.uniform_filter(size=n, mode="constant", cval=0)
 * times n^2, the convention of pysteps' fss; parity with pysteps unpinned.)  rg_contingency_f32, rg_exceedance_sat_i32,
 * rg_fss_sums_i32 and rg_box_fraction_f32 were ADDED; no signature changed, RG_VERSION stays 104.
 *
 * Planes are float32 [n_planes][h][w], row-major, pitch w, no padding; h * w < 2^31 (RG_EINVAL otherwise).  mask (optional, may
 * be NULL) is uint8 of the same shape, non-zero = leave out.
 *   valid      a pixel where neither the forecast nor the observation is NaN and the mask is 0.  +-inf are valid values.
 *   exceeds    a pixel exceeds threshold t when it is valid and `v >= t` in float32.  An invalid pixel exceeds nothing in EITHER
 *              field: the masking is pairwise, so neither side gets credit for it.
 *   thresholds 1 .. RG_MAX_VERIFY_THRESHOLDS finite floats, read on the HOST and passed by value; NaN or inf is RG_EINVAL.
 *   layer      one (plane, threshold) pair, p * n_thr + t.
 *   window     of scale n (1 .. RG_MAX_VERIFY_SCALE, even sizes allowed) at pixel (y, x): rows y - n/2 .. y - n/2 + n - 1
 *              (integer division) and the same span of columns, cut to the plane.  Its count is the number of exceeding pixels
 *              inside; pixels beyond the rim count as 0 (zero padding).
 * All four launch on `stream`, none allocates, none synchronises.  The outputs that are summed into are cleared with
 * hipMemsetAsync on `stream` first.  No float atomics, no workgroup waits for another, no unbounded loop, every index is formed
 * after its bounds test, and a width that is no multiple of 4 or 64 reads nothing outside the plane.
 * ------------------------------------------------------------------------------------------------- */
#define RG_MAX_VERIFY_THRESHOLDS 8
#define RG_MAX_VERIFY_SCALES 16
#define RG_MAX_VERIFY_SCALE 255

/* counts int64 [n_planes][n_thr][3] = (hits: both exceed, false alarms: the forecast only, misses: the observation only) and
 * valid int64 [n_planes] = the valid pixels of the plane pair.  Correct negatives are valid - hits - false alarms - misses.
 * How it runs: a grid-stride pass per plane (blockIdx.y), forecast, observation and mask read once for all thresholds; per
 * threshold three ballots whose popcounts are wave-uniform; the four wavefronts of a workgroup meet in LDS and the workgroup
 * issues one relaxed agent-scope 64-bit integer atomic add per non-zero counter; at most 1024 workgroups per plane.
 * RG_EINVAL before anything touches the device: a null fcst, obs, thresholds_host, counts or valid, n_planes < 1 or > 65535, h
 * or w negative, the size limit, n_thr outside 1 .. 8, a threshold that is not finite, counts or valid overlapping an input or
 * each other.  h == 0 or w == 0 zeroes the outputs and returns. */
int rg_contingency_f32(const float* fcst, const float* obs, const uint8_t* mask, int32_t n_planes, int32_t h, int32_t w,
                       const float* thresholds_host, int32_t n_thr, int64_t* counts, int64_t* valid, rg_stream_t stream);

/* sat int32 [n_planes][n_thr][h][w]: sat[p][t][y][x] = the number of pixels (y', x') of plane p of src with y' <= y, x' <= x that
 * exceed threshold t -- the INCLUSIVE summed-area table.  `partner` (optional, may be NULL) float32 of src's shape supplies only
 * validity: a pixel whose partner is NaN exceeds nothing.  Called once for the forecast with the observation as partner and once
 * the other way round, with the same mask.
 * How it runs: pass 1, one wavefront per row in trips of 64 pixels; the predicate is one bit, so per threshold the inclusive
 * prefix is popcount(ballot & lanes up to me) + carry and carry += popcount(ballot): no shuffles, no LDS; it writes int32 row
 * prefixes.  Pass 2, one thread per (layer, column) adds down the rows in place, the loads of eight rows issued ahead of the adds.
 * RG_EINVAL before anything touches the device: a null src, thresholds_host or sat, n_planes < 1, h or w negative, the size
 * limit, n_thr outside 1 .. 8, a threshold that is not finite, n_planes * n_thr > 65535, sat overlapping an input.  h == 0 or
 * w == 0 returns RG_OK without a launch. */
int rg_exceedance_sat_i32(const float* src, const float* partner, const uint8_t* mask, int32_t n_planes, int32_t h, int32_t w,
                          const float* thresholds_host, int32_t n_thr, int32_t* sat, rg_stream_t stream);

/* sums int64 [n_layers][n_scales][3]: for every layer of the two tables (int32 [n_layers][h][w], as rg_exceedance_sat_i32 writes
 * them) and every scale n, over ALL h * w pixels,
 *     sums[0] = sum (cf - co)^2      sums[1] = sum cf^2      sums[2] = sum co^2
 * with cf and co the window counts of the forecast's and the observation's table: with ya = max(y - n/2, 0) - 1,
 * yb = min(y - n/2 + n - 1, h - 1), likewise xa and xb,  count = S[yb][xb] - S[ya][xb] - S[yb][xa] + S[ya][xa], a corner at index
 * -1 contributing 0.  FSS = 1 - sums[0] / (sums[1] + sums[2]).
 * scales_host: 1 .. RG_MAX_VERIFY_SCALES values in 1 .. RG_MAX_VERIFY_SCALE, read on the HOST and passed by value.
 * OVERFLOW RULE: a window count is at most m = min(n^2, h * w) and each sum at most m^2 * h * w; a shape and scale for which
 * m^2 * h * w can reach 2^63 is RG_EINVAL.  (With n <= 255 the size limit h * w < 2^31 implies it: 65025^2 * 2^31 < 2^63.  The rule
 * is checked on its own all the same, so it keeps holding if either limit moves.)
 * How it runs: one launch spans (strips of pixels, layer, scale); a thread keeps three 64-bit accumulators over its pixels (eight
 * table reads each), a wavefront reduces them with shuffles, the four wavefronts of a workgroup through LDS, and the workgroup
 * issues up to three relaxed agent-scope 64-bit integer atomic adds; at most 1024 workgroups add into one (layer, scale).
 * RG_EINVAL before anything touches the device: null pointers, n_layers < 1, h or w negative, the size limit, n_scales outside
 * 1 .. 16, a scale outside 1 .. 255, the overflow rule, sums overlapping a table.  h == 0 or w == 0 zeroes sums and returns. */
int rg_fss_sums_i32(const int32_t* sat_f, const int32_t* sat_o, int32_t n_layers, int32_t h, int32_t w, const int32_t* scales_host,
                    int32_t n_scales, int64_t* sums, rg_stream_t stream);

/* out float32 [n_layers][h][w] = (float)((double)count / (double)(scale * scale)) with count the window count of `sat` (above):
 * the zero-padded neighbourhood exceedance fraction, "the probability of >= t within scale pixels".  One correctly rounded
 * float64 division and one rounding to float32: NumPy's bits.  One thread per pixel.
 * RG_EINVAL: a null sat or out, n_layers < 1, h or w negative, the size limit, n_layers * h * w >= 2^40, scale outside 1 .. 255,
 * out overlapping sat.  h == 0 or w == 0 returns RG_OK without a launch. */
int rg_box_fraction_f32(const int32_t* sat, int32_t n_layers, int32_t h, int32_t w, int32_t scale, float* out, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Convective / stratiform classification after Steiner, Houze and Yuter 1995: the background reflectivity as the mean of LINEAR
 * reflectivity over a disk, the convective centres (intensity or peakedness over the background), and the convective area as
 * the union of disks whose radius depends on the centre's background.  (No reference counterpart in radar_grid.  The contract
 * is build-defined and restated in NumPy, tests/convection_oracle.py; the relations are those PyART's steiner_conv_strat
 * carries, parity with PyART unpinned.)  rg_echo_table_bytes, rg_echo_table_f32, rg_disk_background, rg_convective_centres_f32,
 * rg_convective_area_workspace_bytes and rg_convective_area_u8 were ADDED; no signature changed, RG_VERSION stays 104.
 *
 * Planes are float32 [n][h][w], row-major, pitch w, no padding; 1 <= n <= 65535 and h * w < 2^31 (RG_EINVAL otherwise).  mask
 * (optional, may be NULL) is uint8 of the same shape, non-zero = leave out.
 *   echo       a pixel that is not NaN, whose mask is 0, and with `dBZ >= min_dbz` in float32.  +inf is an echo.
 *   q          the pixel's linear reflectivity in 2^-16 fixed point: llrint(65536 * 10^(clamp((double)dBZ, -10, 80) / 10)) for an
 *              echo pixel, 0 otherwise; 6554 .. 6.6e12 < 2^43.  10^x is the device's float64 exp10, so q may differ from
 *              NumPy's by one unit at a rounding tie and nowhere else.  Every later sum is an INTEGER sum of these q: exact, and
 *              independent of the order.  Differences of 64-bit row prefixes are exact modulo 2^64 even where a prefix wraps, and
 *              a disk sum is at most 255^2 * 2^43 < 2^59.
 *   footprint  half-widths hw[0 .. ry] on the HOST, passed by value; ry in 0 .. RG_MAX_DISK_RADIUS, every hw[d] in
 *              0 .. RG_MAX_DISK_RADIUS.  At pixel (y, x) it covers columns x - hw[|dy|] .. x + hw[|dy|] of the rows y + dy,
 *              |dy| <= ry, cut to the plane: pixels beyond the rim contribute nothing.  Any table is taken -- it need not be
 *              monotone, so boxes and ellipses work too.
 *   background S int64 = the sum of q over the footprint, N int32 = the echo pixels in it,
 *              bkg = (float)(10 * log10((double)S / (double)N / 65536.0)), NaN where N == 0; defined for EVERY pixel, echo or not.
 *   centre     with v = dBZ and b = bkg as float64 and every operation IEEE float64, unfused: an echo pixel with
 *              `v >= intense`, or `(v - b) >= delta`, delta = peak_a for b < 0 and otherwise c = peak_a - b * b / peak_b where
 *              c > 0, else 0 (Steiner: peak_a = 10, peak_b = 180).  Its class is k = 1 + (the number of edges e with b >= e) over
 *              the n_classes - 1 ascending finite edges, n_classes <= RG_MAX_CONV_CLASSES.  A NaN background makes no centre by
 *              peakedness and class 1 by intensity.  The plane: 0 = no centre, k = a centre of class k.
 *   area       0 = no echo; 2 = an echo pixel with some centre of class k inside footprint k around it (footprints are symmetric:
 *              the pixel lies in the centre's disk); 1 = any other echo pixel (stratiform).  One footprint per class.
 * All launch on `stream`, none allocates, none synchronises.  No atomics, no workgroup waits for another, no unbounded loop, every
 * index is formed after its bounds test, a width that is no multiple of 4 or 64 reads nothing outside the plane, and there is ONE
 * launch path, so the same bits come out of every call.  h == 0 or w == 0 returns RG_OK without a launch.
 * ------------------------------------------------------------------------------------------------- */
#define RG_MAX_DISK_RADIUS 127
#define RG_MAX_CONV_CLASSES 8

/* The bytes of the echo table of n planes of h x w (0 for an empty plane), or a negative rg_status for a shape out of range.
 * The table holds, per row, the exclusive prefixes of q and of the echo count; its layout is opaque (today: one 16-byte entry
 * per pixel plus one per row). */
int64_t rg_echo_table_bytes(int32_t n, int32_t h, int32_t w);

/* Builds the echo table of `dbz` into `table` (16-byte aligned device memory of at least rg_echo_table_bytes bytes).
 * How it runs: one wavefront per row in trips of 64 pixels; the 64-bit prefix of q by a shuffle ladder, the count by one ballot,
 * the carries in scalar registers.
 * RG_EINVAL before anything touches the device: a null dbz or table, the shape limits, a min_dbz that is not finite, the table
 * overlapping an input; RG_EWORKSPACE for table_bytes below the need; RG_EALIGN for a table that is not 16-byte aligned. */
int rg_echo_table_f32(const float* dbz, const uint8_t* mask, int32_t n, int32_t h, int32_t w, float min_dbz, void* table,
                      int64_t table_bytes, rg_stream_t stream);

/* The footprint sums of an echo table: out_sum int64 [n][h][w] = S, out_count int32 = N, out_bkg float32 = bkg; each may be NULL,
 * not all three.  hw_host holds ry + 1 half-widths.  ry = 0 with hw = {0} returns q and the echo flag themselves.
 * How it runs: one wavefront per 64 pixels of a row, four rows per workgroup; per covered row two loads of one 16-byte entry each,
 * whose row distance and half-width are wave-uniform; the sum through the shared core of csrc/rg_disk.hpp.
 * RG_EINVAL: a null table or hw_host, no output, the shape limits, ry or a half-width out of range, an output overlapping the
 * table or another output; RG_EALIGN for a table that is not 16-byte aligned. */
int rg_disk_background(const void* table, int32_t n, int32_t h, int32_t w, const int32_t* hw_host, int32_t ry, int64_t* out_sum,
                       int32_t* out_count, float* out_bkg, rg_stream_t stream);

/* out_class uint8 [n][h][w]: 0, or the class of the convective centre at the pixel (above).  edges_host: n_classes - 1 ascending
 * finite doubles on the HOST (may be NULL for one class).  One thread per pixel.
 * RG_EINVAL: a null dbz, bkg or out_class, the shape limits, n_classes outside 1 .. 8, null edges for more than one class,
 * min_dbz, intense, peak_a, peak_b or an edge that is not finite, peak_b <= 0, a descending edge, out_class overlapping an input. */
int rg_convective_centres_f32(const float* dbz, const uint8_t* mask, const float* bkg, int32_t n, int32_t h, int32_t w, float min_dbz,
                              double intense, double peak_a, double peak_b, const double* edges_host, int32_t n_classes,
                              uint8_t* out_class, rg_stream_t stream);

/* The bytes of the workspace of rg_convective_area_u8 (the row prefixes of the centre count of every class), or a negative
 * rg_status. */
int64_t rg_convective_area_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t n_classes);

/* out uint8 [n][h][w] = the area plane (above) of the centre plane `centres` (values beyond n_classes are no centre).  hw_host
 * int32 [n_classes][RG_MAX_DISK_RADIUS + 1] holds footprint k in row k (its first ry_host[k] + 1 entries are read), ry_host
 * int32 [n_classes].  Echo is judged from dbz, mask and min_dbz as everywhere.
 * How it runs: one wavefront per row writes the per-class row prefixes of "is a centre of class k" (one ballot per class and
 * trip); then per echo pixel the count of every class over its footprint through the SAME core as the background, stopping at
 * the first class that has one.
 * RG_EINVAL: null pointers, the shape limits, n_classes, ry or a half-width out of range, a min_dbz that is not finite, a
 * workspace that is null or not 4-byte aligned, out or the workspace overlapping an operand; RG_EWORKSPACE for a workspace below
 * the need. */
int rg_convective_area_u8(const uint8_t* centres, const float* dbz, const uint8_t* mask, int32_t n, int32_t h, int32_t w,
                          float min_dbz, int32_t n_classes, const int32_t* hw_host, const int32_t* ry_host, void* workspace,
                          int64_t workspace_bytes, uint8_t* out, rg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RADARGRID_HIP_H */
