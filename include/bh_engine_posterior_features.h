/*
 * include/bh_engine_posterior_features.h -- per-site posteriors of structural features of the layered models: libbh_engine.so.
 *
 * An extension of include/bh_engine_posterior_scalars.h, outside the drop-in contract of include/bh_engine.h.  On the rows a
 * bh_posterior handle has loaded it forms a scalar set, BH_SCALARS_FEATURES, whose columns are functionals of every row's step
 * model: layer averages, travel times, the extreme layers, the strongest discontinuities, the first interface above a velocity
 * and the number of interfaces of a depth window.  Every bh_posterior_scalar_* call, bh_posterior_scalar_quantiles and
 * bh_posterior_cov take the set as they take the others.
 *
 * Definitions.  For a loaded row of n layers, vs_j in the row's dtype T and d_j (float64, j = 0..n-2) as in
 * include/bh_engine_posterior.h:
 *   layer j covers [t_j, b_j), t_0 = 0, t_j = d_{j-1}, b_j = d_j, b_{n-1} = +inf (the layer whose vs bh_posterior_columns
 *     returns at a depth inside it);
 *   for a window 0 <= z0 < z1 (finite)  len_j = min(b_j, z1) - max(t_j, z0)  in float64; layer j is in the window where len_j > 0;
 *   jump_k = (double)(T)(vs_{k+1} - vs_k), the Moho rule's subtraction; interface k is in the window where z0 < d_k < z1, strict
 *     on both sides as in the Moho rule;
 *   all sums are float64, sequential in ascending j, starting from 0.0, over the layers in the window; no product or quotient is
 *     contracted into a sum;
 *   a result that is not finite becomes NaN, so the scalar passes never meet an infinity.
 *
 * Kinds, each with the parameters (z0, z1, c) per site:
 *   BH_FEATURE_VSMEAN   1 column    (sum (double)vs_j * len_j) / (z1 - z0)
 *   BH_FEATURE_VSTIME   1 column    (z1 - z0) / sum (len_j / (double)vs_j)
 *   BH_FEATURE_TTS      1 column    sum (len_j / (double)vs_j)
 *   BH_FEATURE_VSMIN    2: value, depth   the layer in the window with the smallest (double)vs_j, the first on ties;
 *   BH_FEATURE_VSMAX    2: value, depth   ... the largest; depth = max(t_j, z0)
 *   BH_FEATURE_DROP     2: depth, jump    the interface in the window with the smallest jump_k, the first on ties, if
 *                                         jump_k < -c (c >= 0); NaN, NaN otherwise
 *   BH_FEATURE_JUMP     2: depth, jump    the interface in the window with the largest jump_k, the first on ties, if jump_k > c
 *                                         (c >= 0); NaN, NaN otherwise
 *   BH_FEATURE_ABOVE    1: depth    d_k of the smallest k in the window with (double)vs_{k+1} > c; NaN if none.  With the Moho's
 *                                   parameters this is column BH_MOHO_DEPTH bit for bit.
 *   BH_FEATURE_NIFACES  1 column    the number of interfaces in the window, as a double; never NaN
 *
 * A site's results are the same bits alone or among other sites, in any row order, on every repeat.  Errors as in
 * bh_engine_posterior.h; BH_EINVAL launches nothing.
 */
#ifndef BH_ENGINE_POSTERIOR_FEATURES_H
#define BH_ENGINE_POSTERIOR_FEATURES_H

#include "bh_engine_posterior_scalars.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BH_SCALARS_FEATURES 4     /* (2 is no set; 3 is BH_SCALARS_DATA of bh_engine_posterior_datafit.h) */
#define BH_FEATURES_MAXKINDS 64   /* F of one call; its columns are at most BH_SCALARS_MAXCOLS */

#define BH_FEATURE_VSMEAN 0
#define BH_FEATURE_VSTIME 1
#define BH_FEATURE_TTS 2
#define BH_FEATURE_VSMIN 3
#define BH_FEATURE_VSMAX 4
#define BH_FEATURE_DROP 5
#define BH_FEATURE_JUMP 6
#define BH_FEATURE_ABOVE 7
#define BH_FEATURE_NIFACES 8

/* Form the FEATURES set from the rows of a load made under bh_posterior_keep_rows.  kind: host [F], 1 <= F <= 64, at most
 * BH_SCALARS_MAXCOLS columns in all; par: host [nsites][F][3] = (z0, z1, c) of every (site, feature), finite, 0 <= z0 < z1, and
 * c >= 0 for DROP and JUMP (BH_EINVAL otherwise, naming the argument).  The columns are laid out feature after feature in the
 * order of kind[], val[c * nrows + r].  found (may be NULL): host [nsites][ncols], the rows with a value in every column. */
int bh_posterior_features(bh_posterior *p, int F, const int32_t *kind, const double *par, int64_t *found);

#ifdef __cplusplus
}
#endif
#endif
