/*
 * include/bh_engine_posterior_cov.h -- posterior covariance and correlation of vs with depth, per site: libbh_engine.so.
 *
 * An extension of include/bh_engine_posterior.h and include/bh_engine_posterior_scalars.h, outside the drop-in contract of
 * include/bh_engine.h.  On the rows a bh_posterior handle has loaded it forms, per site, the mean vector and the population
 * covariance and correlation matrices (ddof = 0) of P = D + Qc columns: the interpolated vs at D depths and Qc chosen columns of
 * one scalar set (Moho depth, crustal vs, attached columns) -- how the depths of a station's profile vary together, and what a
 * tomography node needs beside the mean profile.
 *
 * Columns.  0..D-1 are the vs at dep[0..D) (bh_posterior_columns' sampling); D.. are the columns cols[0..Qc) of the set `set`
 * (BH_SCALARS_MOHO, BH_SCALARS_USER or BH_SCALARS_FEATURES of bh_engine_posterior_features.h; -1 with Qc = 0 for none).  A row with NaN in ANY chosen scalar column is left out of the
 * WHOLE matrix (listwise deletion: the matrix stays symmetric and positive semidefinite): n[site] rows are used, masked[site]
 * left out.  Scalar columns need rows loaded under bh_posterior_keep_rows, as the sets do.
 *
 * Integers.  Per (site, column) a first pass over the rows used finds min, max and the lowest set bit.  L is the smallest
 * exponent >= the lowest set bit's with rint(max * 2^-L) - rint(min * 2^-L) < 2^28 (rint: to nearest, ties to even); exact = 1
 * where it IS the lowest set bit's -- every value is an integer multiple of 2^L -- else 0 and the values are rounded by rint.
 * X0 = rint(min * 2^-L), Y = rint(v * 2^-L) - X0, 0 <= Y < 2^28 (bh_posterior_columns' rule with a tighter width).  A column of
 * zeros only, and every column of a site without rows used, has L = 0, X0 = 0, exact = 1.
 * With Y = H * 2^14 + Lo (BH_COV_LIMB_BITS) the device accumulates, per site and pair of columns i <= j, the three sums
 *   raw0 = sum H_i H_j,  raw1 = sum (H_i Lo_j + Lo_i H_j),  raw2 = sum Lo_i Lo_j,   S_ij = sum Y_i Y_j = raw0 2^28 + raw1 2^14 + raw2
 * on the FP64 matrix cores: inside a chunk of at most 8192 rows every partial sum is an integer below 2^42, exact in float64 in
 * any order; chunks meet in 64-bit integer atomics.  s_i = sum Y_i likewise.  All of n, masked, L, x0, exact, s, raw are pure
 * functions of the multiset of a site's rows: the same bits alone or among other sites, in any row order, from host or device
 * rows, on every repeat.
 *
 * Finished numbers (bh_posterior_cov_finish, host code, 128-bit integers).  N_ij = n S_ij - s_i s_j (|N_ij| < 2^104 for
 * n < 2^24);  mean_i = (s_i / n + X0_i) 2^L_i;  cov_ij = N_ij / n^2 * 2^(L_i + L_j);  corr_ij = N_ij / sqrt(N_ii N_jj), formed in
 * long double, rounded once and clamped to [-1, 1].  The diagonal of corr is exactly 1 where N_ii > 0; a row and column with
 * N_ii = 0 (a constant column, or n <= 1) is NaN in corr and 0 in cov; a site with n = 0 is NaN in mean, cov and corr.  Every
 * finished number is within 1 ulp of the exact rational formed from the integers, both matrices are symmetric bit for bit, and
 * being functions of the integers they inherit their independence of order and company.
 *
 * Every call returns when its results are in host memory.  Errors as in bh_engine_posterior.h; BH_EINVAL and BH_EUNSUPPORTED
 * for an argument launch nothing and write nothing; a value that is not finite is BH_EINVAL and writes nothing.
 */
#ifndef BH_ENGINE_POSTERIOR_COV_H
#define BH_ENGINE_POSTERIOR_COV_H

#include "bh_engine_posterior_scalars.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BH_COV_MAXCOLS 256           /* P = D + Qc of one call */
#define BH_COV_LIMB_BITS 14          /* Y = H * 2^14 + Lo, 0 <= Y < 2^28 */
#define BH_COV_MAXCELLS (1u << 24)   /* nsites * P (P + 1) / 2 of one call */
#define BH_COV_MAXROWS ((1 << 24) - 1) /* rows used per site: n < 2^24 keeps N_ij below 2^104 */

/* dep: host [D], finite, strictly ascending (D may be 0).  set: BH_SCALARS_MOHO / BH_SCALARS_USER / BH_SCALARS_FEATURES, or -1 with Qc = 0.  cols: host
 * [Qc], each a column of the set.  1 <= D + Qc <= BH_COV_MAXCOLS.  Outputs, all host, any may be NULL:
 *   n, masked: int64 [nsites]                        L: int32 [nsites][P]    x0: int64 [nsites][P]    exact: int32 [nsites][P]
 *   s: uint64 [nsites][P]                            raw: uint64 [nsites][P (P + 1) / 2][3], pairs i <= j row-major
 *   mean: float64 [nsites][P]                        cov, corr: float64 [nsites][P][P], full and symmetric
 * BH_EINVAL: a handle without loaded rows, D or Qc negative, P outside 1 .. BH_COV_MAXCOLS, a null dep or cols where needed, a dep
 * that is not finite and strictly ascending, a set that is not MOHO / USER / FEATURES or was not formed, set -1 with Qc > 0, a column outside
 * the set, scalar columns on rows loaded without bh_posterior_keep_rows, nsites * P (P + 1) / 2 above BH_COV_MAXCELLS, a value
 * that is not finite.  BH_EUNSUPPORTED: more than BH_COV_MAXROWS rows of one site. */
int bh_posterior_cov(bh_posterior *p, int D, const double *dep, int set, int Qc, const int32_t *cols, int64_t *n,
                     int64_t *masked, int32_t *L, int64_t *x0, int32_t *exact, uint64_t *s, uint64_t *raw, double *mean,
                     double *cov, double *corr);

/* mean, cov and corr (each may be NULL) from the integers, laid out as above: pure host code, no handle, no GPU.
 * BH_EINVAL: nsites < 1, P outside 1 .. BH_COV_MAXCOLS, a null input, a negative n; BH_EUNSUPPORTED: an n above BH_COV_MAXROWS.
 * Both write nothing.  The integers are trusted to come from bh_posterior_cov (s_i <= n (2^28 - 1), S_ii >= s_i^2 / n). */
int bh_posterior_cov_finish(int nsites, int P, const int64_t *n, const int32_t *L, const int64_t *x0, const uint64_t *s,
                            const uint64_t *raw, double *mean, double *cov, double *corr);

#ifdef __cplusplus
}
#endif
#endif
