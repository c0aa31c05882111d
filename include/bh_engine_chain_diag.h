/*
 * include/bh_engine_chain_diag.h -- order statistics of the chains' recorded series: libbh_engine.so.
 *
 * An extension of include/bh_engine.h, outside its drop-in contract.  It computes on the GPU the sums from which split R-hat,
 * the effective sample size and the integrated autocorrelation time of many chains are formed (bayhunter_amd/diagnostics.py),
 * and the per-chain medians of the reference's outlier rule (Plotting.get_outliers), on the tables of record="device"
 * (include/bh_engine_chain_record.h) where they lie: time-ordered rows, one column per chain.
 *
 * A table is  x[t*ld_t + c*ld_c + q],  t < T rows, c < C chains, q < Q columns; one series per (c, q).  Per series, in float64:
 *   x0  = (double)x_0                          the pivot
 *   d_i = fl((double)x_i - x0)
 *   h   = T / 2 (integer); the first half is i < h, the second half i >= T - h (odd T: the middle sample is in neither)
 *   pass 1:  S1 = sum d_i,  S1a / S1b = the sums of the two halves
 *   pass 2:  m = fl(S1 / T), ma = fl(S1a / h), mb = fl(S1b / h)  (formed on the host between the passes)
 *            M2a = sum over the first half of fl(fl(d_i - ma)^2),  M2b likewise with mb over the second half
 *            P_k = sum_{i < T-k} fl(e_i * e_{i+k}),  e_i = fl(d_i - m),  k = 0..L;  P_k = 0 for k >= T
 * The order of every sum depends on (T, L) only:
 *   S1a, S1b, M2a, M2b: 16 strands -- strand s adds its half's samples i = s (mod 16) in ascending i, starting from 0 -- combined
 *                       (((s0+s1)+(s2+s3))+((s4+s5)+(s6+s7)))+(((s8+s9)+(s10+s11))+((s12+s13)+(s14+s15)));
 *   S1  = (S1a + d_h) + S1b for odd T, S1a + S1b for even T;
 *   P_k: the products added in ascending i, starting from 0.
 * No product is contracted into a sum (-ffp-contract=off).  A series' numbers are therefore the same bits alone or among other
 * series, with other leading dimensions, from host or device memory, and on every repeat.
 *
 * Every call returns when its results are in host memory.  Errors (BH_EINVAL, BH_EHIP, BH_ENOMEM) leave their message in
 * bh_engine_last_error.  BH_EINVAL for an argument launches nothing; BH_EINVAL for the data (a value that is not finite, a model
 * row that is not a row) is found by the first pass.  Neither writes anything to the outputs.
 */
#ifndef BH_ENGINE_CHAIN_DIAG_H
#define BH_ENGINE_CHAIN_DIAG_H

#include "bh_engine.h"
#include "bh_engine_posterior.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BH_DIAG_MAXLAG 2048      /* L */
#define BH_DIAG_MAXCOLS 64       /* Q of one call */
#define BH_DIAG_MAXDEPTHS 63     /* D of bh_chain_diag_models (its nlayers column is the 64th) */
#define BH_DIAG_TILE 256         /* rows the lag kernel takes per step (the halo behind them stays in LDS) */
#define BH_DIAG_LAGBLOCK 1024    /* lags of one workgroup of the lag kernel */
#define BH_DIAG_STRANDS 16

/* memspace BH_HOST: x is a host pointer (the span it covers is copied to the device); BH_DEVICE: a device pointer, read where it
 * lies on stream (NULL: the engine's).  elem_bytes 4 (float32) or 8 (float64).  T >= 1, C >= 1, 1 <= Q <= BH_DIAG_MAXCOLS,
 * 0 <= L <= BH_DIAG_MAXLAG, ld_c >= Q, ld_t >= 1 (elements; the caller's layout: no two series may share an element).
 * x0, s1, s1a, s1b, m2a, m2b: host [C][Q];  p: host [C][Q][L+1].  All must be given. */
int bh_chain_diag_series(bh_engine *e, int memspace, void *stream, int elem_bytes, int64_t T, int C, int Q, int64_t ld_t,
                         int64_t ld_c, const void *x, int L, double *x0, double *s1, double *s1a, double *s1b, double *m2a,
                         double *m2b, double *p);

/* The same for the series derived from model rows  models[t*ld_t + c*ld_c + ..]  of 2*ML values (ML <= BH_POSTERIOR_MAXLAYERS,
 * ld_c >= 2*ML) in the reference's layout [vs_1..vs_n, z_1..z_n, NaN...]:  Q = D + 1 columns, column q < D the vs at depth dep[q]
 * (host, finite, strictly ascending, 0 <= D <= BH_DIAG_MAXDEPTHS) by the rule of bh_engine_posterior.h -- vs[#{j : d_j <= x}],
 * interfaces in the row's dtype, their cumulative sum in float64 --, column D  nlayers = n - 1.  The values are formed in the
 * kernels from the rows; no table of them is written to memory.  A row whose non-NaN values are not a non-empty prefix of even
 * length is BH_EINVAL.  Outputs as above with Q = D + 1. */
int bh_chain_diag_models(bh_engine *e, int memspace, void *stream, int elem_bytes, int64_t T, int C, int ML, int64_t ld_t,
                         int64_t ld_c, const void *models, int D, const double *dep, int L, double *x0, double *s1, double *s1a,
                         double *s1b, double *m2a, double *m2b, double *p);

/* The two middle order statistics of every chain's column of  x[t*ld_t + c*ld_c]  (t < T, c < C; memspace, stream, elem_bytes as
 * above): lo[c] = the value of rank (T-1)/2, hi[c] = of rank T/2 (equal for odd T), as float64 -- numpy.median is their mean in
 * the table's dtype.  A radix selection on the ordered bit patterns: exact.  A value that is not finite is BH_EINVAL.
 * lo, hi: host [C]. */
int bh_chain_diag_medians(bh_engine *e, int memspace, void *stream, int elem_bytes, int64_t T, int C, int64_t ld_t, int64_t ld_c,
                          const void *x, double *lo, double *hi);

#ifdef __cplusplus
}
#endif
#endif
