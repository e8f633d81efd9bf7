/* radargrid_hydro.h -- hydrometeor classification in the polar domain: the texture of a field along the ray and a table-driven
 * fuzzy-logic classifier of every gate: the sixth header of libradargrid_hip.so.
 *
 * The two entry points declared here are compiled into the SAME library as those of the other five headers (csrc/rg_hydro.hip)
 * and follow the conventions of radargrid_phase.h: device pointers unless a name ends in _host, the stream last, every argument
 * validated and RG_EINVAL returned before anything touches the device, rg_last_error() text beginning with the function's name,
 * no allocation, no host synchronisation and no memset node (the calls can be captured into a hipGraph).  They live in a header
 * of their own, bound from the table `_native.HYDRO_SIGNATURES`, so that the other five headers and their tables stay
 * byte-identical: rg_polar_texture_f32 and rg_fuzzy_classify_f32 were ADDED; no signature changed, RG_VERSION stays 104.
 *
 * The classifier is the fuzzy logic of Park et al. (2009) in its general form: trapezoidal membership functions per (class,
 * variable), tabulated per bin of a condition variable (Z there), a weighted mean of the memberships of the additive variables
 * times the product of those of the multiplicative ones.  Which classes, variables and vertices is the TABLE's business; the
 * kernel knows none of them.  Every sum of the texture is an integer in 2^-10 fixed point and every float step of both entry
 * points is stated, so the outputs are bit-reproducible and the tests hold them EQUAL to the NumPy restatement of exactly these
 * formulas (tests/hydro_oracle.py).  (No reference counterpart in radar_grid.  Parity with the WSR-88D HCA, wradlib and CSU
 * RadarTools is unpinned.)
 *
 * Common definitions:
 *   Arrays are [R][G] row-major with pitch G: one row is one ray, R >= 1 rays of 0 <= G <= RG_PHASE_MAX_GATES gates,
 *   R * G < 2^31.  The sweeps of a volume are simply stacked.  Every MISSING float32 output is the quiet NaN 0x7FC00000.
 *   G == 0 returns RG_OK without a launch.  Float arithmetic is unfused, in the order written; an int64 -> double conversion
 *   rounds to nearest even; sqrt and / are the correctly rounded IEEE operations.
 *   Each call is ONE launch of workgroups of 256 that STRIDE over their work (tiles, or gates), so no count of rays is refused
 *   for the size of a launch.
 */
#ifndef RADARGRID_HYDRO_H
#define RADARGRID_HYDRO_H

#include "radargrid_hip.h"   /* rg_stream_t, the status codes */
#include "radargrid_phase.h" /* RG_PHASE_MAX_GATES */

#ifdef __cplusplus
extern "C" {
#endif

#define RG_HYDRO_TEXTURE_SHIFT 10    /* the fixed point of the texture: q = x * 2^10 */
#define RG_HYDRO_MAX_ABS 8192        /* |x| beyond it is not valid, so that |q| <= 2^23 */
#define RG_HYDRO_MAX_HALF_GATES 63   /* the texture window is at most 127 gates */
#define RG_HYDRO_TEXTURE_TILE 512    /* gates of one ray a workgroup of rg_polar_texture_f32 takes at a time */
#define RG_HYDRO_MAX_VARS 8          /* variables of the classifier */
#define RG_HYDRO_MAX_CLASSES 16      /* classes */
#define RG_HYDRO_MAX_BINS 32         /* bins of the condition variable */
#define RG_HYDRO_MAX_CELLS 1024      /* B * C * V at most: 48 KB of cells in LDS */
#define RG_HYDRO_UNCLASSIFIED 0      /* cls of a gate without a class; class c is c + 1 */

/* ---------------------------------------------------------------------------------------------------
 * 1  Texture: the standard deviation and the mean of a field in a window along the ray.
 *
 * x      float32 [R][G];  mask (optional, may be NULL) uint8 [R][G], non-zero = leave the gate out.
 * A gate is VALID when x is finite, |x| <= RG_HYDRO_MAX_ABS and its mask is 0.  Its fixed-point value is
 * q = llrint(1024 * (double)x): exact to 2^-10 of the unit, ties to even, |q| <= 2^23.
 * The window of gate i is the gates max(0, i - L) .. min(G - 1, i + L) of the same ray, L = half_gates in
 * 1 .. RG_HYDRO_MAX_HALF_GATES.  Over the VALID gates of the window, as exact integers (int64):
 *   N = the count,  Sq = sum q,  Sqq = sum q * q
 *   D = N * Sqq - Sq * Sq
 * Bounds: N <= 127 < 2^7 and q * q <= 2^46, so Sqq < 2^53 and N * Sqq < 2^60; |Sq| <= 127 * 2^23 < 2^30, so Sq * Sq < 2^60.
 * D = N^2 times the variance of the q: never negative (Cauchy-Schwarz), below 2^60.  Everything is exact in int64, in any
 * order of summation.
 * The result is DEFINED where N >= min_valid (min_valid in 1 .. 127) and, with centre_only != 0, gate i itself is valid.  There
 *   sd   = (float)((sqrt((double)D) / (double)N) / 1024.0)          the population standard deviation
 *   mean = (float)(((double)Sq / (double)N) / 1024.0)
 * elsewhere both are NaN.  count (optional uint16 [R][G]) = N, written at EVERY gate, defined or not.
 * sd and mean are each optional, at least one is required.  No output may overlap an input or another output.
 * How it runs: one launch, no table in HBM.  A workgroup of 256 takes a tile of RG_HYDRO_TEXTURE_TILE = 512 gates of one ray
 * plus a halo of RG_HYDRO_MAX_HALF_GATES = 63 gates on either side (of which it loads L), stages validity, q and q * q once and
 * builds their tile-relative prefixes in LDS with the shuffle ladder; every lane then takes two prefix reads per sum for each of
 * its two gates.  Exact, since all three are integers (prefix of q * q < 638 * 2^46 < 2^56).  The workgroups stride over the
 * R * ceil(G / 512) tiles.
 * RG_EINVAL before any launch: a null x; sd and mean both NULL; R < 1; G outside 0 .. RG_PHASE_MAX_GATES; R * G >= 2^31;
 * half_gates or min_valid outside its range; an output overlapping an input or another output. */
int rg_polar_texture_f32(const float* x, const uint8_t* mask, int32_t R, int32_t G, int32_t half_gates, int32_t min_valid,
                         int32_t centre_only, float* sd, float* mean, uint16_t* count, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * 2  Fuzzy-logic classification of every gate, driven by a table of trapezoids.
 *
 * vars_host   V pointers (1 <= V <= RG_HYDRO_MAX_VARS), read on the host and passed by value, none NULL.  Variable v is float32
 *             on the device: [R][G], or, when bit v of per_sweep_bits is set, a table [R / rays_per_sweep][G] indexed by
 *             (ray / rays_per_sweep, gate) -- one row per sweep (temperature: a value per sweep and range, not per ray).
 *             rays_per_sweep >= 1 and divides R; per_sweep_bits and required_bits have no bit at or above V.
 * kind_host   V values read on the host: 0 = additive, 1 = multiplicative.  At least one variable is additive.
 * mask        (optional, may be NULL) uint8 [R][G]: non-zero = the gate is not classified.
 * cond_var    -1 .. V - 1: the variable whose value chooses the BIN of a gate, and edges_host, B - 1 finite ascending doubles
 *             (may be NULL when B == 1) read on the host, 1 <= B <= RG_HYDRO_MAX_BINS.  The bin is the number of edges e with
 *             x_cond >= (float)e, compared in float32 (as the half-window classes of rg_phidp_fit_f32).  cond_var == -1
 *             requires B == 1: every gate is in bin 0.
 * cells       float64 [B][C][V][6] on the device, 8-byte aligned: (x1, x2, x3, x4, r, f) per (bin, class, variable),
 *             1 <= C <= RG_HYDRO_MAX_CLASSES, B * C * V <= RG_HYDRO_MAX_CELLS.  The kernel TRUSTS the table (the host side
 *             builds it: x1 <= x2 <= x3 <= x4, r = 1 / (x2 - x1) and f = 1 / (x4 - x3) where that is finite, else 0).
 * weights_host  C * V doubles [C][V] read on the host, finite and >= 0.   min_score  a double, finite and >= 0.
 *
 * Per gate.  x_v = (double)var_v; variable v is PRESENT where its value is finite.  The gate is NOT CLASSIFIED where its mask is
 * non-zero, a variable with its bit in required_bits is not present, or (cond_var >= 0) the condition variable is not present.
 * Otherwise, with the cells of the gate's bin, all in float64, the membership of x in (x1, x2, x3, x4, r, f) is
 *   0                            if x < x1 or x > x4
 *   1                            if x2 <= x <= x3
 *   min((x - x1) * r, 1.0)       if x1 <= x < x2             min(t, 1.0) = t < 1.0 ? t : 1.0
 *   min((x4 - x) * f, 1.0)       if x3 < x <= x4
 * (infinite vertices give open shoulders), and per class c, v ascending:
 *   A += w[c][v] * m  and  W += w[c][v]     over the PRESENT additive variables, both from 0.0
 *   P *= m                                  over the PRESENT multiplicative ones, from 1.0
 *   score_c = (W > 0 ? A / W : 0.0) * P
 * The winner is the class of the largest score, the lowest class among equals; the runner-up is the same among the OTHER
 * classes.  (A score that is NaN -- weights whose sum overflows -- neither wins nor runs up.)
 *   cls    (required, uint8 [R][G]) = winner + 1, or RG_HYDRO_UNCLASSIFIED = 0 where the gate is not classified, the best score
 *          is 0 (or no score is a number), or the best score is < min_score
 *   score  (optional, float32 [R][G]) = (float)best, NaN where cls == 0
 *   second (optional, uint8 [R][G]) = runner-up + 1; 0 where cls == 0, C == 1, or no other score is a number
 * No output may overlap an input, the table or another output.
 * How it runs: one launch, one thread per gate, workgroups of 256 striding over the gates.  Each workgroup stages the cell table
 * in LDS once (at most 48 KB: three workgroups per CU); the V values of a gate stay in registers; a lane reads the cells of its
 * own bin; no division per cell (the reciprocals come with the table), one float64 division per class.  The weights, the edges
 * (as float32) and the flags travel in the kernel's argument block.
 * RG_EINVAL before any launch: a null vars_host, kind_host, weights_host, cells or cls, or a null entry of vars_host; V, C or B
 * outside its range; B * C * V > RG_HYDRO_MAX_CELLS; a kind that is not 0 or 1, or no additive variable; bits at or above V; the
 * size limits; rays_per_sweep < 1 or not dividing R; cond_var outside -1 .. V - 1, or -1 with B > 1; a null edges_host with
 * B > 1, an edge that is not finite or edges that descend; a weight or a min_score that is not finite or negative; a refused
 * overlap.  RG_EALIGN: cells not 8-byte aligned. */
int rg_fuzzy_classify_f32(const float* const* vars_host, const int32_t* kind_host, int32_t V, int32_t per_sweep_bits,
                          int32_t required_bits, int32_t rays_per_sweep, const uint8_t* mask, int32_t R, int32_t G,
                          int32_t cond_var, const double* edges_host, int32_t B, const double* cells, int32_t C,
                          const double* weights_host, double min_score, uint8_t* cls, float* score, uint8_t* second,
                          rg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RADARGRID_HYDRO_H */
