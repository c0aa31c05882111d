/*
 * include/bh_engine_posterior_datafit.h -- posterior data fits of many sites: libbh_engine.so.
 *
 * An extension of include/bh_engine_posterior_scalars.h, outside the drop-in contract of include/bh_engine.h.  On the rows a
 * bh_posterior handle has loaded after bh_posterior_keep_rows(p, 1) it provides what BayHunter's
 * PlotFromStorage.plot_bestdatafits / plot_bestmodels compute one model at a time -- the model of least joint misfit of every
 * chain, converted back to layers -- and one step more: the synthetic data of EVERY loaded row as a scalar set, whose
 * per-site column statistics and order statistics are the posterior predictive band of every period and time sample.
 *
 *   bh_posterior_layers       rows [r0, r1) -> nlay, h, vp, vs, rho in the layout bh_evaluate_sites takes, and their site
 *   bh_posterior_best         the input row of the first least misfit of every (site, chain)
 *   bh_posterior_data_fill    a forward batch's ymod / err -> the columns of the set BH_SCALARS_DATA (NaN = masked)
 *   bh_posterior_scalar_quantiles   up to 8 order statistics of every (site, column) of any set in one read per radix pass
 *   bh_posterior_scalar_gather      the values of given loaded rows of a set
 *
 * The layer rule, for a loaded row [vs_1..vs_n, z_1..z_n] of dtype T (Model.get_vp_vs_h and plot_bestdatafits' rho, in the
 * dtypes numpy computes them in):  h_j = (double)zd_j - (double)zd_{j-1} (zd_{-1} = 0; the kept zd_j = (z_j + z_{j+1}) / 2 in
 * T), h_{n-1} = 0;  vp_j = vs_j * (T)vpvs in T;  with a mantle rule (mantle_vs > 0) from the first layer with vs_j >=
 * (T)mantle_vs downward vp_j = vs_j * (T)mantle_vpvs;  rho_j = vp_j * (T)0.32 + (T)0.77 in T, the product rounded before the
 * sum.  All widened to float64; layers n .. ML-1 of a row are written as 0.
 *
 * Results are the same bits in any row order, alone or among other sites, on every repeat.  Errors as in
 * bh_engine_posterior.h; BH_EINVAL launches nothing (except where a device array must be read to find the fault, stated below).
 */
#ifndef BH_ENGINE_POSTERIOR_DATAFIT_H
#define BH_ENGINE_POSTERIOR_DATAFIT_H

#include "bh_engine_posterior_scalars.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BH_SCALARS_DATA 3          /* the third scalar set (id 2 is no set) */
#define BH_DATAFIT_MAXCOLS 4096    /* columns (ldy) of the DATA set */
#define BH_QUANTILES_MAXRANKS 8    /* order statistics per column of one bh_posterior_scalar_quantiles call */

/* Loaded rows [r0, r1) (0 <= r0 <= r1 <= the loaded rows, in the order the load left them: grouped by site) as layers.
 * vpvs: one value per row of the loaded INPUT, vpvs_elem 4 (float32) or 8 (float64) bytes, vpvs_stride elements apart, host
 * (memspace BH_HOST: copied to the device on every call -- a caller with many batches passes a device array) or device; read
 * at the row's index in the input and cast to the row's dtype.  stream: as bh_posterior_load (device memspace).
 * mantle_vs / mantle_vpvs: host [nsites], mantle_vs <= 0 = no rule at that site; both NULL = no rule anywhere.
 * Outputs (device): nlay, site int32 [r1 - r0]; h, vp, vs, rho float64, layer j of row r0 + b at [j * stride_l + b], j = 0 ..
 * ML-1 (ML of the load; stride_l >= r1 - r0).  Asynchronous on the stream (the copy of a host vpvs is waited for); the mantle
 * table stays on the device between calls and is uploaded again only where it differs from the last call's. */
int bh_posterior_layers(bh_posterior *p, int64_t r0, int64_t r1, int memspace, void *stream, int vpvs_elem, int64_t vpvs_stride,
                        const void *vpvs, const double *mantle_vs, const double *mantle_vpvs, int32_t *nlay, double *h,
                        double *vp, double *vs, double *rho, int64_t stride_l, int32_t *site);

/* The best fit of every (site, chain): chain (int32, 0 <= chain < nchains) and misfit (misfit_elem 4 or 8 bytes) hold one
 * value per row of the loaded input, chain_stride / misfit_stride elements apart, host or device (memspace, stream as above).
 * Rows the load left out take no part.  best: host int64 [nsites][nchains], the input-row index of the first least misfit of
 * the pair (numpy.argmin over the chain's rows in input order; -0.0 equals 0.0), -1 where the pair has no row.  pos (may be
 * NULL): host int64 [nsites][nchains], that row's position among the loaded rows (for bh_posterior_scalar_gather), -1 likewise.
 * Two integer atomicMin passes: the ordered key of the misfit, then the input index over the rows that hold that key.
 * BH_EINVAL: nchains < 1 or nsites * nchains > 2^24; a host chain id out of range (any input row; nothing launched); a chain id
 * out of range or a NaN misfit in a loaded row (found by the first pass; best and pos are not written). */
int bh_posterior_best(bh_posterior *p, int nchains, int memspace, void *stream, const int32_t *chain, int64_t chain_stride,
                      int misfit_elem, const void *misfit, int64_t misfit_stride, int64_t *best, int64_t *pos);

/* The DATA set: Q = ldy columns over the loaded rows, val[q * nrows + r].  A call takes the synthetics ymod [nb][ldy] and err
 * [nb] (device) that bh_evaluate_sites wrote for the loaded rows [r0, r0 + nb) and writes them transposed.  ncol: host
 * [nsites][nt], the samples site s has in target t (0: the site lacks the slot); target t's column block is as wide as its
 * largest count over the sites, block after block, and the blocks must add up to ldy.  NaN is written where the row's err != 0,
 * where the column lies beyond the site's own count in its target, and where the site lacks the target.
 * Calls go in order: r0 = 0 starts the set again (Q = ldy, 1 .. BH_DATAFIT_MAXCOLS) and puts the tables of the fill on the
 * device, where they stay; every following call continues where the last one ended with the same ldy and the same ncol
 * (BH_EINVAL otherwise) and only enqueues its kernel -- ymod and err may be written again by work enqueued after it on the
 * same stream.  The set exists (for the bh_posterior_scalar_* calls) once all loaded rows are filled, and that call returns
 * after the device is done.  failed (may be NULL): host [nsites], written by that last call: the rows with
 * err != 0.  stream: the stream ymod and err were written on (NULL: the engine's).
 * The transposition goes through an LDS tile of 64 rows x 64 columns, padded to 65. */
int bh_posterior_data_fill(bh_posterior *p, void *stream, int64_t r0, int64_t nb, int ldy, const double *ymod, const int32_t *err,
                           int nt, const int32_t *ncol, int64_t *failed);

/* Order statistics of every (site, column) of a set (MOHO, USER or DATA) whose bh_posterior_scalar_stats has run since it was
 * formed (it holds the counts and the float32-exactness the select needs; BH_EINVAL otherwise).  R = 1 .. BH_QUANTILES_MAXRANKS
 * ranks per column; rank: host [nsites][ncols][R], each below the column's count (a column of count 0 takes rank 0 only).
 * lower / upper: host [nsites][ncols][R], the 64-bit ordered keys (bh_posterior_columns' map) of the order statistic `rank`
 * and of the next one above it (equal to lower where rank is the last; both 0 where the count is 0).
 * One radix kernel serves all R ranks of a column in the same read of the column: R x 256 LDS counters per workgroup and a
 * prefix per rank, a key counted for rank r where it matches r's prefix (ranks whose prefixes are still equal share counters);
 * 4 passes where every column is float32-exact, 8 otherwise, each column sitting out the passes it does not need; then one
 * multi-rank pass for the next keys.  Device memory: nsites * ncols * R KiB of counters (BH_ENOMEM where that fails). */
int bh_posterior_scalar_quantiles(bh_posterior *p, int set, int R, const uint32_t *rank, uint64_t *lower, uint64_t *upper);

/* The values of n loaded rows of a set: pos host [n] (0 <= pos < the loaded rows), out host [n][ncols]. */
int bh_posterior_scalar_gather(bh_posterior *p, int set, int64_t n, const int64_t *pos, double *out);

#ifdef __cplusplus
}
#endif
#endif
