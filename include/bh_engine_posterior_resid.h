/*
 * include/bh_engine_posterior_resid.h -- posterior residuals of many sites: libbh_engine.so.
 *
 * An extension of include/bh_engine_posterior_datafit.h, outside the drop-in contract of include/bh_engine.h.  Where
 * bh_posterior_data_fill keeps the synthetics of every loaded row, bh_posterior_resid_fill keeps what says whether their residuals
 * look like the noise the row itself assumed: per (row, target slot) the bias and rms of the residual, its amplitude against the
 * row's sigma, its lag-1 correlation against the row's corr, and its autocorrelation function at the lags 1 .. L -- as one more
 * scalar set, BH_SCALARS_RESID, which every pass behind a scalar set (bh_posterior_scalar_stats, _quantiles, _gather, ...) serves
 * unchanged.  BayHunter's own check is plot_rfcorr: the residual of the single best model above one random noise realisation,
 * compared by eye.
 *
 * Definitions, for a loaded row of site s and slot t with n = ncol[s][t] samples (i = 0 .. n-1 within the slot's column block):
 *   e_i = ymod_i - yobs_i                (the reference's ydiff)
 *   u_i = fl(e_i * g_i)                  (g: 1 everywhere where the call brings none)
 * All arithmetic is float64 and nothing is contracted: every product is rounded before it is added.
 *   S(x)  a sum over i ascending in 64 strands: strand j (0 .. 63) starts at +0.0 and takes the i = j (mod 64) one after the other;
 *         then s_j = s_j + s_{j xor w} for w = 32, 16, 8, 4, 2, 1 (every strand at once), and S = s_0.  The order of every sum
 *         depends on (n, l) only.
 *   A_l = S(fl(u_i * u_{i+l})) over i < n - l
 *
 *   column  name          value
 *   0       bias          S(e_i) / n
 *   1       rms           sqrt(S(fl(e_i * e_i)) / n)            (the reference's get_rms; sqrt correctly rounded)
 *   2       sigma_ratio   sqrt(A_0 / n) / sigma_t               (about 1 under any of the four laws if the noise model is right)
 *   3       corr          corr_t, the row's own, copied
 *   4       corr_excess   acf_1 - corr_t
 *   4 + l   acf_l         A_l / A_0,  l = 1 .. L
 *
 * NaN (the quiet NaN 0x7ff8000000000000) is written, and nothing else is ever non-finite: in every column of a row with err != 0;
 * in every column of a slot the site lacks (n = 0); in acf_l where l >= n (and hence in corr_excess where n = 1); in every quotient
 * with A_0 = 0; and in place of any result that is not finite (sigma_t <= 0 gives no finite ratio; a non-finite noise value).
 *
 * A row's columns are the same bits alone or among other sites, in any row order, for any split into batches, from host or device
 * noise, on every repeat.  Errors as in bh_engine_posterior.h; BH_EINVAL launches nothing and leaves the set unformed.
 */
#ifndef BH_ENGINE_POSTERIOR_RESID_H
#define BH_ENGINE_POSTERIOR_RESID_H

#include "bh_engine_posterior_datafit.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BH_SCALARS_RESID 5     /* the fifth scalar set */
#define BH_RESID_MAXLAG 32     /* lags of the autocorrelation function */
#define BH_RESID_FIXED 5       /* the columns of a slot before its autocorrelation function */

/* The RESID set: Q = nt * (BH_RESID_FIXED + L) columns over the loaded rows, val[q * nrows + r]; slot t holds the columns
 * t * (BH_RESID_FIXED + L) onwards.  A call takes the synthetics ymod [nb][ldy] and err [nb] (device) that bh_evaluate_sites wrote
 * for the loaded rows [r0, r0 + nb), exactly as bh_posterior_data_fill does (ldy, nt, ncol: the column blocks of the DATA set),
 * and may be made beside it on the same batch.
 * L: the lags, 1 .. BH_RESID_MAXLAG.  yobs: host [nsites][ldy], every site's observed data in that column layout (read at the
 * site's own counts only).  g: host [nsites][ldy] in the same layout, or NULL for 1.0 everywhere.
 * noise: one value row per row of the loaded INPUT, noise_ld >= 2 * nt elements apart, (corr_t, sigma_t) of slot t at 2t, 2t + 1;
 * noise_elem 4 (float32) or 8 (float64) bytes; noise_memspace BH_HOST or BH_DEVICE; read at the loaded row's index in the input and
 * widened to double.  A host table is put on the device by the call that starts the fill, and the following calls read that copy;
 * a device table is read by every call's kernel on `stream`.
 * Calls go in order: r0 = 0 starts the set again and puts ncol, yobs and g (and a host noise table) on the device, where they stay;
 * every following call continues where the last one ended with the same ldy, nt, ncol, L, yobs, g and the same kind of noise table
 * (memspace, element size, noise_ld) -- BH_EINVAL otherwise -- and only enqueues its kernel: ymod and err may be written again by
 * work enqueued after it on the same stream.  The set exists (for the bh_posterior_scalar_* calls) once all loaded rows are filled,
 * and that call returns after the device is done.  failed (may be NULL): host [nsites], written by that last call: the rows with
 * err != 0.  stream: the stream ymod and err were written on (NULL: the engine's).
 * BH_EINVAL: L out of range; Q beyond BH_DATAFIT_MAXCOLS; noise_ld < 2 * nt or an element size that is neither 4 nor 8; what
 * bh_posterior_data_fill refuses in ldy, nt, ncol and the rows; calls out of order; tables that differ from the first call's; null
 * arguments.
 * A wavefront takes a (row, slot): its lanes are the 64 strands, u_{i+l} comes from the current and the next 64 samples by one lane
 * shuffle per lag, the butterfly is lane shuffles, and 64 rows' columns are transposed through an LDS tile as in
 * bh_posterior_data_fill. */
int bh_posterior_resid_fill(bh_posterior *p, void *stream, int64_t r0, int64_t nb, int ldy, const double *ymod, const int32_t *err,
                            int nt, const int32_t *ncol, int L, const double *yobs, const double *g, int noise_memspace,
                            int noise_elem, int64_t noise_ld, const void *noise, int64_t *failed);

#ifdef __cplusplus
}
#endif
#endif
