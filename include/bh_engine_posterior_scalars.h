/*
 * include/bh_engine_posterior_scalars.h -- per-site posteriors of scalar quantities: libbh_engine.so.
 *
 * An extension of include/bh_engine_posterior.h, outside the drop-in contract of include/bh_engine.h.  On the rows a
 * bh_posterior handle has loaded it computes what BayHunter's PlotFromStorage.plot_moho_crustvel_tradeoff and
 * plot_posterior_likes / _misfits / _nlayers / _vpvs / _noise / _others compute from a station's posterior: per site the
 * count, min, max, median, exact integer sums for mean and std, and 1-D and 2-D histograms of scalar columns.
 *
 * A scalar set is a table of Q float64 columns over the loaded rows; a NaN masks a row for that column.  Two sets:
 *   BH_SCALARS_MOHO  bh_posterior_moho: moho, vslast, vscrust, vsjump (columns 0..3) of every row with a Moho, NaN else.
 *   BH_SCALARS_USER  bh_posterior_attach: caller columns, one value row per row of the loaded input, and optionally
 *                    nlayers = n - 1 as the last column.
 * A set lives until the next bh_posterior_load or the next call that forms it again.  Usage: bh_posterior_keep_rows(p, 1),
 * bh_posterior_load, then bh_posterior_moho and / or bh_posterior_attach, then any number of the bh_posterior_scalar_* calls.
 *
 * The Moho rule, for a row [vs_1..vs_n, z_1..z_n]:  zd_j = (z_j + z_{j+1}) / 2 (row dtype), h_j = (double)zd_j -
 * (double)zd_{j-1} (zd_{-1} = 0), ifaces_j = the sequential float64 sum of h_0..h_j (j = 0..n-2).  The Moho is the smallest
 * k in 0..n-2 with lo < ifaces_k < hi and (double)vs_{k+1} > mohovs; moho = ifaces_k, vslast = (double)vs_k, vsjump =
 * (double)(vs_{k+1} - vs_k) (subtracted in the row's dtype), vscrust = S / ifaces_k with S the sum of (double)vs_j * h_j,
 * j = 0..k, in numpy.sum's order (sequential below 8 terms; else 8 strided accumulators over the whole blocks of 8, combined
 * ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the rest added sequentially), no product contracted into a sum.
 *
 * Every call returns when its results are in host memory; a site's results are the same bits alone or among other sites,
 * in any row order, on every repeat.  Errors as in bh_engine_posterior.h; BH_EINVAL launches nothing.
 */
#ifndef BH_ENGINE_POSTERIOR_SCALARS_H
#define BH_ENGINE_POSTERIOR_SCALARS_H

#include "bh_engine_posterior.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BH_SCALARS_MOHO 0
#define BH_SCALARS_USER 1
#define BH_SCALARS_MAXCOLS 64      /* caller columns of bh_posterior_attach */

#define BH_MOHO_DEPTH 0
#define BH_MOHO_VSLAST 1
#define BH_MOHO_VSCRUST 2
#define BH_MOHO_VSJUMP 3

/* on != 0: the following bh_posterior_load calls of the handle keep what the scalar sets need beside the rows -- every row's
 * index in the loaded input (8 bytes) and its zd_j in the row's dtype (ML values).  bh_posterior_moho and bh_posterior_attach
 * are BH_EINVAL on rows loaded without it.  Off by default: the calls of bh_engine_posterior.h pay nothing for it. */
int bh_posterior_keep_rows(bh_posterior *p, int on);

/* Form the MOHO set.  lo, hi, mohovs: host [nsites], finite, 0 <= lo < hi (BH_EINVAL otherwise).
 * found (may be NULL): host [nsites], the rows with a Moho. */
int bh_posterior_moho(bh_posterior *p, const double *lo, const double *hi, const double *mohovs, int64_t *found);

/* Form the USER set: Q (0..BH_SCALARS_MAXCOLS) columns of elem_bytes 4 (float32) or 8 (float64) values, value row i (ld
 * elements apart) belonging to row i of the input of the last bh_posterior_load (values of rows the load left out are
 * ignored).  memspace / stream as in bh_posterior_load.  with_nlayers != 0 adds the column nlayers = n - 1 as column Q.
 * Q = 0 needs with_nlayers. */
int bh_posterior_attach(bh_posterior *p, int memspace, void *stream, int elem_bytes, int Q, int64_t ld, const void *values,
                        int with_nlayers);

/* The columns of a set: 4 for MOHO, Q (+ 1) for USER; BH_EINVAL for a set that was not formed. */
int bh_posterior_scalar_cols(bh_posterior *p, int set, int32_t *ncols);

/* Per site and column of a set (all host, [nsites][ncols]): count = the rows with a value, nnan = the rows with NaN, kmin /
 * kmax = the ordered keys of min and max (the 64-bit map of bh_posterior_columns), scale / x0 / exact / sums[..][6] = the exact
 * integer sums of bh_posterior_columns over the rows with a value, median[..][2] (may be NULL) = the 64-bit ordered keys of
 * the ranks (count-1)/2 and (count-1)/2 + 1 (the second equals the first where count is 1; both 0 where it is 0).
 * A column whose values are all float32-exact is selected on 32-bit keys (half the passes); the keys returned are the
 * 64-bit ones.  A value that is not finite is BH_EINVAL. */
int bh_posterior_scalar_stats(bh_posterior *p, int set, int64_t *count, int64_t *nnan, uint64_t *kmin, uint64_t *kmax,
                              int32_t *scale, int64_t *x0, int32_t *exact, uint64_t *sums, uint64_t *median);

/* numpy.histogram counts of column col: site s's edges are edges[edge_off[s] .. edge_off[s+1]) (host, finite, ascending,
 * at least 2; edge_off[0] = 0), the bin rule of bh_posterior_hist.  counts: host, site s's bins at sum_{t<s} nbins_t (at
 * most BH_POSTERIOR_MAXCOUNTS in all). */
int bh_posterior_scalar_hist(bh_posterior *p, int set, int col, const int64_t *edge_off, const double *edges,
                             uint32_t *counts);

/* numpy.histogram2d counts of column colx against column coly over the rows that have both: per-site edges on both axes as
 * above.  counts: host, site s's [nx_s][ny_s] at sum_{t<s} nx_t * ny_t (at most BH_POSTERIOR_MAXCOUNTS cells in all).
 * argmax (may be NULL): host [nsites], the first largest cell of the flattened [nx][ny] counts (numpy.argmax). */
int bh_posterior_scalar_hist2d(bh_posterior *p, int set, int colx, int coly, const int64_t *xedge_off, const double *xedges,
                               const int64_t *yedge_off, const double *yedges, uint32_t *counts, int64_t *argmax);

#ifdef __cplusplus
}
#endif
#endif
