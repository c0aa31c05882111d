/*
 * include/bh_engine_chain_diag_features.h -- the structural features of the chains' recorded models as time-ordered series:
 * libbh_engine.so.
 *
 * An extension of include/bh_engine_chain_diag.h and include/bh_engine_posterior_features.h, outside the drop-in contract of
 * include/bh_engine.h.  bh_posterior_features forms the features of rows a bh_posterior handle has loaded -- scattered by site, their
 * time order lost.  This call forms the same columns from the store where it lies, [rows][chains][2*ML], as one series per chain (or
 * per gathered series, include/bh_engine_chain_diag_ladders.h), in the layout bh_chain_diag_series reads: what split R-hat, the
 * effective sample size and a Monte-Carlo standard error of a Moho depth or a sediment thickness are taken of.
 *
 * models: the table x[t*ld_t + c*ld_c + i], i < 2*ML, float32 or float64, as bh_chain_diag_models takes it.  A row is
 * [vs_1..vs_n, z_1..z_n, NaN..]; its layers are those of include/bh_engine_posterior.h -- zd_j = (z_j + z_{j+1}) / 2 in the row's
 * type, d_j the float64 running sum of (double)zd_j - (double)zd_{j-1}.  kind, par, the column layout (feature after feature in the
 * order of kind[]: col0[f]), the argument checks and their messages are those of bh_posterior_features; series k takes the
 * parameters of its site, par[site[k]].
 *
 * A row may lack a column (a drop, a jump, an interface above a velocity: the rule gives NaN).  The sums of bh_chain_diag_series
 * refuse what is not finite, so the value and the presence leave as two tables:
 *   value[t][k][q]    the column's value; +0.0 where the row lacks it
 *   present[t][k][q]  1.0f where the row has it, 0.0f where it lacks it
 *   missing[k][q]     the number of rows of series k that lack column q
 *
 * The contract: value / present are, bit for bit, the FEATURES columns bh_posterior_features forms for the same rows with the same
 * parameters -- the same device code walks both (bayhunter_amd/csrc/feature_rule.h).  The result is the same alone or among other
 * series, in host or device memory, with any leading dimensions, on every repeat.
 *
 * With sel, series k reads chain sel[t*ld_sel + k] at row t: the index is clamped into [0, C) before it is an address, and an index
 * outside is BH_EINVAL ("index"), as in bh_engine_chain_diag_ladders.h; rows of chains not selected at a row are never read.
 *
 * Refusals.  BH_EINVAL for an argument launches nothing.  BH_EINVAL for the data -- a selection index outside [0, C), a non-NaN row
 * value that is not finite, a row whose non-NaN values are not a non-empty prefix of even length -- is found by a first pass over
 * the rows before anything is written.  Neither writes to an output.
 */
#ifndef BH_ENGINE_CHAIN_DIAG_FEATURES_H
#define BH_ENGINE_CHAIN_DIAG_FEATURES_H

#include "bh_engine_chain_diag_ladders.h"
#include "bh_engine_posterior_features.h"

#ifdef __cplusplus
extern "C" {
#endif

/* memspace, stream, elem_bytes, T, C, ML, ld_t, ld_c, models: as bh_chain_diag_models.  K, sel, ld_sel: as bh_chain_diag_models_sel;
 * sel NULL: K == C and series k reads chain k.  site: host [K], the series' site in 0..nsites-1.  F, kind (host [F]), par (host
 * [nsites][F][3]): as bh_posterior_features.  value (float64), present (float32): [T][K][ncols] in the memspace of models, element
 * (t, k, q) at t*ld_out_t + k*ld_out_k + q, ld_out_k >= ncols.  missing: host [K][ncols].  T * K stays below 2^36. */
int bh_chain_diag_features(bh_engine *e, int memspace, void *stream, int elem_bytes, int64_t T, int C, int ML, int64_t ld_t,
                           int64_t ld_c, const void *models, int K, const int32_t *sel, int64_t ld_sel, int nsites,
                           const int32_t *site, int F, const int32_t *kind, const double *par, double *value, float *present,
                           int64_t ld_out_t, int64_t ld_out_k, int64_t *missing);

#ifdef __cplusplus
}
#endif
#endif
