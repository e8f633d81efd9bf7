/* radargrid_phase.h -- differential phase in the polar domain: the third header of libradargrid_hip.so.
 *
 * The three entry points declared here are compiled into the SAME library as those of radargrid_hip.h and
 * radargrid_ensemble.h (csrc/rg_phase.hip) and follow the same conventions: device pointers unless a name ends in _host, the
 * stream last, every argument validated and RG_EINVAL returned before anything touches the device, rg_last_error() text
 * beginning with the function's name, no allocation, no host synchronisation and no memset node (so the calls can be captured
 * into a hipGraph).  They live in a header of their own, bound from the table `_native.PHASE_SIGNATURES`, so that the other two
 * headers and their tables stay byte-identical: rg_phidp_unfold_f32, rg_phidp_fit_f32 and rg_attenuation_phidp_f32 were ADDED;
 * no signature changed, RG_VERSION stays 104.
 *
 * (No reference counterpart in radar_grid; the tests pin the kernels to the NumPy restatement of exactly these formulas,
 * tests/phase_oracle.py.  Parity with PyART / wradlib is unpinned.)
 *
 * Common to all three:
 *   Arrays are [R][G] row-major with pitch G: one row is one ray, R >= 1 rays of 0 <= G <= RG_PHASE_MAX_GATES gates,
 *   R * G < 2^31.  The sweeps of a volume are simply stacked: rays never interact.  Every MISSING float32 output is the quiet
 *   NaN 0x7FC00000.  G == 0 returns RG_OK without a launch.  Float arithmetic is unfused, in the order written.
 *   Each call is ONE launch of workgroups of 256, and a launch holds fewer than 2^32 work-items, so a call takes at most
 *   RG_PHASE_MAX_WORKGROUPS workgroups: rg_phidp_unfold_f32 and rg_attenuation_phidp_f32 use one per four rays
 *   (R <= 4 * RG_PHASE_MAX_WORKGROUPS = 67108860), rg_phidp_fit_f32 one per ray and 512 gates
 *   (R * ceil(G / 512) <= RG_PHASE_MAX_WORKGROUPS: 16777215 rays of up to 512 gates).  More rays are refused with RG_EINVAL:
 *   split the volume by rays, which never interact.
 */
#ifndef RADARGRID_PHASE_H
#define RADARGRID_PHASE_H

#include "radargrid_hip.h" /* rg_stream_t, the status codes */

#ifdef __cplusplus
extern "C" {
#endif

#define RG_PHASE_MAX_GATES 32768   /* gates of one ray */
#define RG_PHASE_MAX_CLASSES 4     /* half-window classes of rg_phidp_fit_f32 */
#define RG_PHASE_MAX_HALF_WINDOW 255
#define RG_PHASE_MAX_WORKGROUPS 16777215 /* 2^24 - 1 workgroups of 256: what one launch holds */
#define RG_PHASE_MAX_ABS_PHI 16384 /* degrees: |phi| beyond it is left out of a fit, so that 65536 * phi fits 2^30 */

/* ---------------------------------------------------------------------------------------------------
 * 1  Unfold PHIDP across its +-wrap (Itoh's unwrapping along the ray).
 *
 * phidp  float32 [R][G] degrees;  mask (optional, may be NULL) uint8 [R][G], non-zero = leave the gate out.
 * wrap   the folding interval in degrees (360, or 180), finite and > 0, with (float)(0.5 * wrap) finite and > 0.
 * A gate is VALID when its value is finite and its mask is 0.  Walk the valid gates of a ray in ascending order; p is the
 * previous valid gate of the same ray, however far back:
 *   d    = phidp[i] - phidp[p]                      one float32 subtraction
 *   half = (float)(0.5 * wrap)
 *   k_i  = -1 if d > half, +1 if d < -half, else 0; the first valid gate of a ray has k = 0
 *   K_i  = the sum of k_j over the valid gates j <= i of the ray (int32)
 *   out[i]   = (float)((double)phidp[i] + (double)K_i * wrap)       one float64 multiply, one add, one rounding
 *   folds[i] = K_i            (optional int32 [R][G])
 * Invalid gates get NaN in out and 0 in folds.  d exactly +-half is no fold.
 * The limit of the method: a noise excursion beyond wrap / 2 between neighbouring valid gates is taken for a fold and shifts
 * the rest of the ray by wrap.  Mask the gates of low RHOHV (rg_gate_mask_f32) and despeckle BEFORE this call.
 * In place: out == phidp is allowed (each gate is read before it is written); any other overlap of out or folds with phidp,
 * mask or each other is refused.
 * How it runs: one wavefront per ray in trips of 64 gates; "the previous valid value" is a ballot plus one shuffle from the
 * nearest lower set lane, K a shuffle ladder; the last valid value and K are carried from trip to trip in scalar registers.
 * RG_EINVAL before any launch: a null phidp or out; R < 1; G outside 0 .. RG_PHASE_MAX_GATES; R * G >= 2^31; a wrap that is
 * not finite and > 0 (or whose float32 half is not); a refused overlap. */
int rg_phidp_unfold_f32(const float* phidp, const uint8_t* mask, int32_t R, int32_t G, double wrap, float* out, int32_t* folds,
                        rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * 2  Windowed least-squares line through the unfolded PHIDP: the smoothed PHIDP and KDP.
 *
 * phi    float32 [R][G], the unfolded PHIDP.  A gate is VALID when phi is finite and |phi| <= RG_PHASE_MAX_ABS_PHI; its
 *        fixed-point value is q = llrint(65536 * (double)phi), an integer with |q| <= 2^30.
 * dbz    (optional, may be NULL) float32 [R][G]: chooses the half-window of gate i.
 * n_classes 1 .. RG_PHASE_MAX_CLASSES;  half_windows_host[k] in 1 .. RG_PHASE_MAX_HALF_WINDOW for k < n_classes;
 * edges_host  n_classes - 1 finite ascending doubles (may be NULL when n_classes == 1).  Both are read on the host and passed
 *        by value.  The class of gate i is the number of edges e with dbz[i] >= (float)e, compared in float32; a NULL dbz or
 *        a NaN dbz[i] counts no edge: class 0.  L = half_windows_host[class].
 * The window of gate i is the gates max(0, i - L) .. min(G - 1, i + L); j = the gate index minus i.  Over the VALID gates of
 * the window, as exact integers (int64):
 *   N = the count,  Sj = sum j,  Sjj = sum j^2,  Sq = sum q,  Sjq = sum j * q
 *   den = N * Sjj - Sj^2,  num = N * Sjq - Sj * Sq            (|N * Sjq| and |Sj * Sq| stay below 2^57)
 * The fit is DEFINED where N >= min_valid (min_valid in 2 .. 511), den > 0 and, if centre_only != 0, gate i itself is valid;
 * with centre_only == 0 gaps inside an echo are filled.  Where defined, all float64 and in this order:
 *   s     = (double)num / (double)den
 *   kdp   = (float)(s * scale)
 *   phi_s = (float)((((double)Sq - s * (double)Sj) / (double)N) / 65536.0)
 * elsewhere both are NaN.  scale is finite; the host passes 500 / (65536 * gate_spacing_m), which makes kdp one-way deg/km.
 *   count (optional uint16 [R][G]) = N, written at EVERY gate, defined or not.
 * kdp and phi_s are each optional, at least one is required.  How the sums are formed does not matter to the result: they are
 * integers.  No output may overlap an input or another output.
 * How it runs: no table in HBM.  A workgroup takes a tile of 512 gates of one ray plus a halo of 255 gates on either side,
 * builds tile-relative prefixes of (valid, t, t^2, q, t * q), t = the position in the tile, in LDS with the shuffle ladder,
 * and every lane then takes two prefix reads per sum and re-centres them on its own gate -- exact, since all are integers.
 * RG_EINVAL before any launch: a null phi; kdp and phi_s both NULL; the size limits; n_classes, a half-window or min_valid
 * outside its range; a null half_windows_host, or a null edges_host with n_classes > 1; an edge that is not finite or edges that
 * descend; a scale that is not finite; a refused overlap. */
int rg_phidp_fit_f32(const float* phi, int32_t R, int32_t G, const float* dbz, const double* edges_host,
                     const int32_t* half_windows_host, int32_t n_classes, int32_t min_valid, int32_t centre_only, double scale,
                     float* kdp, float* phi_s, uint16_t* count, rg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * 3  Path-integrated attenuation by the linear-PHIDP method, with a monotone path.
 *
 * phi_s  float32 [R][G], the smoothed PHIDP (NaN where it is not defined).
 * phi0   (optional, may be NULL) float32 [R]: the system offset of each ray.  Where it is NULL or NaN the origin of the ray
 *        is its first non-NaN phi_s.
 * alpha, beta   dB per degree, finite and >= 0;  max_dphi   degrees, finite, with cap = (float)max_dphi > 0.
 *   e_i = phi_s[i] - origin            one float32 subtraction; a NaN result (a NaN phi_s, inf - inf) counts as -inf
 *   m_i = min(max(+0, max over j <= i of e_j), cap)        float32; never negative, never -0, never NaN, non-decreasing in i
 *   a ray without any non-NaN phi_s has m = 0 everywhere
 *   dphi (optional)  = m
 *   pia  (optional)  = (float)(alpha * (double)m)
 *   dbz_out          = dbz + (float)(alpha * (double)m)         one float32 add: a NaN dbz stays NaN
 *   zdr_out          = zdr + (float)(beta * (double)m)          zdr and zdr_out: both or neither
 * In place: dbz_out == dbz and zdr_out == zdr are allowed; any other overlap of an output with an input or another output is
 * refused.
 * How it runs: one wavefront per ray in trips of 64 gates; "the first defined value" is a ballot and one shuffle, the running
 * maximum a shuffle ladder (max is exact in any order), both carried from trip to trip in scalar registers.
 * RG_EINVAL before any launch: a null phi_s, dbz or dbz_out; zdr without zdr_out or the reverse; the size limits; alpha, beta
 * or max_dphi outside its range; a refused overlap. */
int rg_attenuation_phidp_f32(const float* phi_s, const float* phi0, int32_t R, int32_t G, double alpha, double beta,
                             double max_dphi, const float* dbz, const float* zdr, float* dbz_out, float* zdr_out, float* pia,
                             float* dphi, rg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RADARGRID_PHASE_H */
