/* radargrid_shear.h -- azimuthal shear and radial divergence of the Doppler velocity by local linear least squares (LLSD), and
 * the small median filter that precedes it: the fifth header of libradargrid_hip.so.
 *
 * The two entry points declared here are compiled into the SAME library as those of the other four headers (csrc/rg_shear.hip)
 * and follow the conventions of radargrid_velocity.h: device pointers unless a name ends in _host, the stream last, every
 * argument validated and RG_EINVAL returned before anything touches the device, rg_last_error() text beginning with the
 * function's name, no allocation, no host synchronisation and no memset node (the calls can be captured into a hipGraph).  They
 * live in a header of their own, bound from the table `_native.SHEAR_SIGNATURES`, so that the other four headers and their
 * tables stay byte-identical: rg_polar_median_f32 and rg_velocity_llsd_f32 were ADDED; no signature changed, RG_VERSION stays
 * 104.
 *
 * The method is the LLSD of Smith & Elmore (2004) as used by Mahalik et al. (2019): a plane v ~ v0 + al * i + be * j is fitted
 * to the velocities of a window of (ray, gate) neighbours, i the ray offset and j the gate offset from the centre gate; al
 * scaled by the arc length of one ray step is the azimuthal shear, be scaled by the gate spacing the radial divergence.  It is
 * restated so that every sum the fit rests on is an integer in 2^-16 m/s fixed point: the outputs are bit-reproducible and the
 * tests hold them EQUAL to the NumPy restatement of exactly these formulas (tests/shear_oracle.py).  (No reference counterpart
 * in radar_grid.  Parity with WDSS-II / LROSE / PyART is unpinned.)
 *
 * Two limits of the restatement.  The fit is in INDEX coordinates: all gates of a window share the centre gate's arc length per
 * ray step (the true arc length grows with range across the window), and the rays of a sweep are taken as equally spaced.
 *
 * Common definitions:
 *   A volume is vel float32 [S][R][G]: S >= 1 sweeps of R >= 1 rays of G >= 0 gates, row-major, S * R * G < 2^31.
 *   mask (optional, may be NULL) uint8 of the same shape: non-zero leaves the gate out.
 *   A gate is VALID when its value is finite, |v| <= RG_VELOCITY_MAX_ABS (radargrid_velocity.h) and its mask is 0.
 *   q = llrint(65536 * (double)v): the fixed-point value, exact, |q| <= 2^30.
 *   Sweeps never interact.  wrap_rays != 0: a sweep is a closed circle in azimuth, ray -1 is ray R - 1 OF THE SAME SWEEP;
 *   without it rays outside 0 .. R - 1 are in no window.  Gates outside 0 .. G - 1 are never in a window.
 *   Every MISSING float32 output is the quiet NaN 0x7FC00000, and so is any NaN a formula below produces (from a table entry
 *   that is not finite).  Float arithmetic is unfused, in the order written; an int64 -> double conversion rounds to nearest
 *   even.
 *   G == 0 returns RG_OK without a launch.
 */
#ifndef RADARGRID_SHEAR_H
#define RADARGRID_SHEAR_H

#include "radargrid_hip.h"      /* rg_stream_t, the status codes */
#include "radargrid_velocity.h" /* RG_VELOCITY_MAX_ABS */

#ifdef __cplusplus
extern "C" {
#endif

#define RG_SHEAR_MEDIAN_MAX_HALF 2   /* the median window is at most 5 x 5 */
#define RG_SHEAR_MAX_HALF_RAYS 16    /* the LLSD window is at most 33 rays ... */
#define RG_SHEAR_MAX_HALF_GATES 16   /* ... by 33 gates */
#define RG_SHEAR_MAX_WINDOW 1089     /* 33 * 33: the largest count */

/* ---------------------------------------------------------------------------------------------------
 * 1  The median pre-filter.
 *
 * The window of gate (s, a, g): rays a - half_rays .. a + half_rays, gates g - half_gates .. g + half_gates.  n = the number
 * of its VALID gates.  Where n >= min_valid and (the centre gate is valid or centre_only == 0)
 *   out = the value of rank floor((n - 1) / 2) of the valid values in ascending order
 * -- the LOWER median, a selection and never an average: the output bits are the bits of an input.  -0.0 and +0.0 compare
 * equal; where both are in a window either may be returned.  Elsewhere out = NaN.
 * One thread per gate: the window (at most 25 values) is held in registers and sorted by a fixed network of compare-exchanges.
 * RG_EINVAL before any launch: a null vel or out; the sizes; half_rays or half_gates outside 0 .. RG_SHEAR_MEDIAN_MAX_HALF or
 * both 0; wrap_rays != 0 with 2 * half_rays + 1 > R; min_valid outside 1 .. 25; out overlapping vel or mask. */
int rg_polar_median_f32(const float* vel, const uint8_t* mask, int32_t S, int32_t R, int32_t G, int32_t half_rays,
                        int32_t half_gates, int32_t wrap_rays, int32_t min_valid, int32_t centre_only, float* out,
                        rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * 2  The LLSD: azimuthal shear, radial divergence and the fitted (smoothed) velocity.
 *
 * half_rays int32 [G] and az_scale double [G] are tables on the device, one entry per gate index (range).  The window of gate
 * (s, a, g) uses ka = min(max(half_rays[g], 0), max_half_rays), clamped on the device, and covers rays a - ka .. a + ka and
 * gates g - half_gates .. g + half_gates.  W = (2 * ka + 1) * (2 * half_gates + 1) is the FULL window size, whether or not an
 * edge clips it.
 *
 * Over the VALID gates of the window, i the ray offset and j the gate offset, as exact int64:
 *   n = sum 1   Si = sum i   Sj = sum j   Sii = sum i*i   Sij = sum i*j   Sjj = sum j*j   Sq = sum q   Siq = sum i*q   Sjq = sum j*q
 *   A = n*Sii - Si^2     B = n*Sij - Si*Sj     C = n*Sjj - Sj^2
 *   P = n*Siq - Si*Sq    Q = n*Sjq - Sj*Sq     D = A*C - B*B
 * Bounds, with both half-widths at most 16: n <= 33 * 33 = 1089 < 2^11.  sum over a full window of i*i is 33 * 2 * (1^2 + ..
 * + 16^2) = 33 * 2992 = 98736, so n*Sii <= 1089 * 98736 < 2^27 and 0 <= A, C < 2^29; |B| <= sqrt(A*C) (Cauchy-Schwarz), so
 * 0 <= D <= A*C < 2^57.  |q| <= 2^30 and sum |i| over a full window is 33 * 2 * 136 = 8976, so |Sq| <= 1089 * 2^30 < 2^41,
 * |Siq|, |Sjq| <= 8976 * 2^30 < 2^44, n*|Siq| < 2^55 and |Si*Sq| <= 8976 * 1089 * 2^30 < 2^54: |P|, |Q| < 2^56.  Everything is
 * exact in int64, in any order of summation.
 *
 * The fit is DEFINED where all of these hold: n >= min_valid;  n * 65536 >= min_fraction_q16 * W;  D > 0;  and, with
 * centre_only != 0, the centre gate is valid.  There, all in float64 and in this order:
 *   al         = ((double)P * (double)C - (double)Q * (double)B) / (double)D          per ray step
 *   be         = ((double)Q * (double)A - (double)P * (double)B) / (double)D          per gate step
 *   az_shear   = (float)(al * az_scale[g])
 *   divergence = (float)(be * range_scale)
 *   vel_s      = (float)(((((double)Sq - al * (double)Si) - be * (double)Sj) / (double)n) / 65536.0)
 * Elsewhere the three are NaN.  count (optional, uint16) = n is written at EVERY gate.
 * With az_scale[g] = 1 / (65536 * r_g * dtheta_rad) and range_scale = 1 / (65536 * gate_spacing_m) both products are in 1/s.
 *
 * How it runs: ONE launch, no intermediate in device memory.  A workgroup of 256 takes 32 gates of 40 consecutive rays plus a
 * halo of H rays on either side, H the largest ka among ITS OWN 32 gates (ka falls with range: most tiles have a halo of one or
 * two rays).  For every (ray, gate) of tile and halo it forms the five range-window sums (n, Sj, Sjj, Sq, Sjq) -- they do not
 * depend on the centre ray -- in LDS: every value of tile and halo is loaded into registers first (one trip to memory for all
 * of them), the fixed-point values of 32 rays at a time are staged in LDS, a thread takes 4 consecutive gates of one ray, sums
 * the first window and slides it.  An entry is 24 bytes (n, Sj in 16 bits, Sjj in 32, Sq and
 * Sjq in 64), kept as three arrays so that consecutive lanes read consecutive 8-byte words.  Each lane then combines its column
 * of 2 * ka + 1 entries with weights 1, i, i*i into the nine sums and does the fit.  Static LDS: 65352 bytes, so two workgroups fit a CU.
 *
 * RG_EINVAL before any launch: a null vel, half_rays or az_scale; all of az_shear, divergence and vel_s null; the sizes;
 * max_half_rays outside 1 .. RG_SHEAR_MAX_HALF_RAYS; half_gates outside 1 .. RG_SHEAR_MAX_HALF_GATES; wrap_rays != 0 with
 * 2 * max_half_rays + 1 > R; min_valid outside 3 .. RG_SHEAR_MAX_WINDOW; min_fraction_q16 outside 0 .. 65536; a range_scale
 * that is not finite; an output overlapping an input or another output.  RG_EALIGN: az_scale not 8-byte aligned. */
int rg_velocity_llsd_f32(const float* vel, const uint8_t* mask, int32_t S, int32_t R, int32_t G, const int32_t* half_rays,
                         const double* az_scale, int32_t max_half_rays, int32_t half_gates, double range_scale,
                         int32_t wrap_rays, int32_t min_valid, int32_t min_fraction_q16, int32_t centre_only, float* az_shear,
                         float* divergence, float* vel_s, uint16_t* count, rg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RADARGRID_SHEAR_H */
