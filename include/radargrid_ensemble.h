/* radargrid_ensemble.h -- probabilistic nowcasts: the second header of libradargrid_hip.so.
 *
 * The two entry points declared here are compiled into the SAME library as those of radargrid_hip.h (csrc/rg_ensemble.hip) and
 * follow the same conventions: device pointers unless a name ends in _host, the stream last, every argument validated and
 * RG_EINVAL returned before anything touches the device, rg_last_error() text beginning with the function's name, no
 * allocation and no host synchronisation (so the calls can be captured into a hipGraph).  They live in a header of their own,
 * bound from the table `_native.ENSEMBLE_SIGNATURES`, so that radargrid_hip.h and `_native.SIGNATURES` stay byte-identical:
 * rg_ensemble_exceedance_f32 and rg_ensemble_histogram_u8 were ADDED; no signature changed, RG_VERSION stays 104.  Folding
 * this header into radargrid_hip.h later changes no ABI.
 *
 * (No reference counterpart in radar_grid; the tests pin both kernels to the NumPy restatement of exactly these formulas,
 * tests/ensemble_oracle.py.)
 */
#ifndef RADARGRID_ENSEMBLE_H
#define RADARGRID_ENSEMBLE_H

#include "radargrid_hip.h" /* rg_stream_t, rg_motion_lattice, the status codes, RG_MAX_LEADS, RG_MAX_VERIFY_THRESHOLDS */

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------
 * Ensemble exceedance probabilities: "what is the probability of at least 35 dBZ here in 30 minutes".  An ensemble of
 * n_members semi-Lagrangian extrapolations of ONE plane, member m displaced at lead l by the common displacement of
 * rg_advect_f32 plus its own shift, is thresholded and counted per pixel in one pass: the member planes are never stored.
 *
 * Motion, its sign, its units and rg_motion_lattice are those of "Echo motion and nowcasts" (radargrid_hip.h); the two
 * sampling rules are those of rg_advect_f32 (the kernels share csrc/rg_motion_field.hpp and csrc/rg_sample.hpp, so with all
 * shifts zero every member IS the plane rg_advect_f32 writes, bit for bit).
 * ------------------------------------------------------------------------------------------------- */
#define RG_MAX_MEMBERS 64

/* src        float32 [h][w], one plane, row-major, pitch w; h * w < 2^31.
 * motion     float32 [ny][nx][2] on the device and `lattice`: those of rg_advect_f32, ALL FINITE (the caller's duty).
 * leads_host n_leads in 0 .. RG_MAX_LEADS finite doubles in units of the interval, read on the host, passed by value.
 * substeps   1 .. 16.      method   0 nearest, 1 bilinear.
 * shifts     float64 [n_leads][n_members][2] = (sy, sx) in pixels ON THE DEVICE: member m's extra displacement at lead l
 *            (up to 16 KB: too large to pass by value).  It must be finite: the caller's duty.  A NaN shift makes that member
 *            MISSING at every pixel of that lead, never a fault.
 * n_members  1 .. RG_MAX_MEMBERS.
 * thresholds_host   n_thr in 1 .. RG_MAX_VERIFY_THRESHOLDS finite floats, read on the host, passed by value.
 * min_members       1 .. n_members.
 *
 * Per pixel p = (y, x) and lead l, everything float64, unfused, in this order:
 *   1  d exactly as in rg_advect_f32: "motion at a point" once at p, then "displacement" with lead / substeps; the base
 *      position is b = p - d.
 *   2  member m samples src at (b_y - sy[l][m], b_x - sx[l][m]) by the rule of `method`:
 *        nearest   iy = floor(fy + 0.5), ix = floor(fx + 0.5), the value copied bit for bit; outside the plane: NaN;
 *        bilinear  the four taps (y0,x0), (y0,x0+1), (y0+1,x0), (y0+1,x0+1), NaN and outside taps missing, wsum and vsum in
 *                  float64, v = (float)(vsum / wsum) if wsum >= 0.5, else NaN.
 *   3  a sample is MISSING when it is NaN: the position outside the plane (nearest), a weight sum below 0.5 (bilinear), or a
 *      NaN value copied or computed.  Every other sample is PRESENT; +-inf are values.
 *   4  n_valid = the number of present members.
 *   5  cnt[t] = the number of present members with v >= thresholds[t], compared in float32.
 * Outputs (each may be NULL, but not all of them):
 *   prob     float32 [n_leads][n_thr][h][w] = (float)((double)cnt[t] / (double)n_valid) where n_valid >= min_members, else NaN
 *   counts   uint8   [n_leads][n_thr][h][w] = cnt[t]                      (0 .. n_members, whatever min_members)
 *   members  uint8   [n_leads][h][w]        = n_valid
 *   mean     float32 [n_leads][h][w]        = (float)(S / (double)n_valid), S = 0.0 + (double)v_m over the present members in
 *                                             ascending m; NaN where n_valid < min_members
 * How it runs: one thread per pixel and lead (blockIdx.y = the lead); the base position is computed once per thread, not once
 * per member; the member loop reads its shifts at wave-uniform addresses; n_valid, the eight counts (eight 8-bit fields of one
 * 64-bit register: a count reaches 64) and S stay in registers, and all output planes of the pixel are written after the
 * loop.  The member samples of neighbouring pixels overlap, so the plane is served from cache.  No atomics, no workgroup waits
 * for another, every output is bit-reproducible.
 * RG_EINVAL before any launch: a null src, motion, leads_host (with n_leads > 0), shifts (with n_leads > 0) or
 * thresholds_host; all four outputs NULL; h or w negative; the size limit; n_leads, substeps, method, n_members, n_thr or
 * min_members outside its range; a lead, a threshold or a lattice member that is not finite; a step <= 0; ny or nx < 1; an
 * output overlapping src, motion, shifts or another output.  h == 0, w == 0 or n_leads == 0 returns RG_OK without a launch. */
int rg_ensemble_exceedance_f32(const float* src, int32_t h, int32_t w, const float* motion, rg_motion_lattice lattice,
                               const double* leads_host, int32_t n_leads, int32_t substeps, int32_t method,
                               const double* shifts, int32_t n_members, const float* thresholds_host, int32_t n_thr,
                               int32_t min_members, float* prob, uint8_t* counts, uint8_t* members, float* mean,
                               rg_stream_t stream);

/* The counts a probability forecast is verified from: how often k of M members exceeded a threshold, and how often the
 * observation then did.
 * counts   uint8 [n_planes][n_thr][h][w] and members uint8 [n_planes][h][w]: as rg_ensemble_exceedance_f32 writes them (a plane
 *          is a lead, or a lead of one of several scans);  obs  float32 [n_planes][h][w];  mask (optional, may be NULL) uint8
 *          of obs's shape, non-zero = leave the pixel out.
 * n_members   M in 1 .. RG_MAX_MEMBERS;  thresholds_host as above;  1 <= n_planes <= 65535;  h * w < 2^31.
 * A pixel is VALID when obs is not NaN there, the mask is 0, members == M (a complete ensemble) and every one of its n_thr
 * counts is <= M.  An index is formed only after that test, so counts above M (which rg_ensemble_exceedance_f32 never writes)
 * are left out, never a fault.
 *   hist    int64 [n_planes][n_thr][M + 1][2]:  hist[p][t][k][o] = the valid pixels of plane p with counts[p][t] == k and
 *           o = (obs >= thresholds[t]) in float32 (+-inf are values)
 *   valid   int64 [n_planes] = the valid pixels;  for every p and t, the sum of hist[p][t] over k and o equals valid[p]
 * How it runs: blockIdx.y = the plane, at most 512 workgroups per plane walk its pixels grid-stride; per-workgroup bins in
 * LDS (int32, at most 8 * 65 * 2 * 4 = 4160 bytes), flushed with relaxed agent-scope 64-bit integer atomic adds, zero bins
 * skipped.  hist and valid are cleared on `stream` first, by a kernel (a memset node of a captured graph has been seen to
 * zero on the first replay only: csrc/rg_common.hpp).  Integer adds only: every count is exact in any order.
 * RG_EINVAL before any launch: a null counts, members, obs, thresholds_host, hist or valid; n_planes outside 1 .. 65535; h or
 * w negative; the size limit; n_members or n_thr outside its range; a threshold that is not finite; hist overlapping valid, or
 * either overlapping an input.  h == 0 or w == 0 zeroes hist and valid and returns. */
int rg_ensemble_histogram_u8(const uint8_t* counts, const uint8_t* members, const float* obs, const uint8_t* mask,
                             int32_t n_planes, int32_t h, int32_t w, int32_t n_members, const float* thresholds_host,
                             int32_t n_thr, int64_t* hist, int64_t* valid, rg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RADARGRID_ENSEMBLE_H */
