/*
 * include/bh_engine_chain_rank.h -- the rank transform of the chains' recorded series: libbh_engine.so.
 *
 * An extension of include/bh_engine.h, outside its drop-in contract.  It forms on the GPU the three tables from which the
 * rank-normalised split R-hat, the folded split R-hat and the bulk and tail effective sample sizes of Vehtari et al. (2021) are
 * computed (bayhunter_amd/diagnostics.py: rank_series, rank_models, rank_convergence) with the sums of bh_engine_chain_diag.h.
 *
 * A table is  x[t*ld_t + c*ld_c + q],  t < T rows, c < C chains, q < Q columns, as in bh_engine_chain_diag.h.  group[c] (host)
 * in [0, G) is the pool the chain's samples are ranked in (its site); -1 leaves the chain out (an outlier).  The pool of group g
 * and column q is every (t, c) with group[c] == g: N_g = m_g * T values  v = (double)x,  -0.0 taken as +0.0, compared as numbers.
 * With all counts and divisions in integers:
 *   lt(v) = #{w in pool : w < v},   eq(v) = #{w in pool : w == v}  (itself included),   R2 = 2 lt + eq + 1   (twice the average
 *   rank, in [2, 2N])
 *   bulk  :  z  = zt[zoff[g] + R2]
 *   tail  :  lo = lt <= (N - 1) / 20 ? 1 : 0,   hi = lt <= (19 (N - 1)) / 20 ? 1 : 0     -- the indicators of x <= q_0.05 and
 *            x <= q_0.95 for the linear-interpolation quantiles, stated without a floating quantile
 *   folded:  med = fl(fl(s_(N-1)/2 + s_N/2) * 0.5) of the sorted pool s_0 <= .. <= s_N-1 (numpy.median of the float64 pool),
 *            f = |fl(v - med)|,  ltf, eqf, R2f as above over the f of the pool,  zf = zt[zoff[g] + R2f]
 * zt is the caller's table of normal scores, read and never computed here: for a pool of N the entries zoff[g] .. zoff[g] + 2N
 * (diagnostics.rank_table(N): zt_N[R2] = normal_quantile((R2/2 - 3/8) / (N + 1/4)); entries 0 and 1 are never read).  Groups of
 * equal N may share their entries.
 *
 * Every output is a function of integer counts and of one table lookup: the same bits alone or among other pools and columns,
 * with other leading dimensions, from host or device memory, and on every repeat.
 *
 * Outputs, in the memspace of x (device pointers for BH_DEVICE, host pointers for BH_HOST), with o = t*ld_out_t + c*ld_out_c:
 *   z[o + q], zf[o + q] (float64),   tail[2*o + 2*q] = lo, tail[2*o + 2*q + 1] = hi (float32)  -- contiguous tables [T][C][Q] and
 *   [T][C][2Q] have ld_out_c = Q, ld_out_t = C*Q.
 * Any of them may be NULL; without zf the second sort is not run.  Elements of chains with group[c] == -1 get 0 in every output
 * and are never read for a pool.
 *
 * How: per column the pool elements of all groups become order-preserving unsigned keys (32-bit for a float32 table, 64-bit for
 * float64) with their element index t*C + c, a segmented least-significant-digit radix sort (8 bits per pass, BH_RANK_TILE keys
 * per workgroup and pass) orders every pool, lt and eq come from the tie runs of the sorted keys; the folded keys are always
 * 64-bit and are sorted again.  The call walks the columns: its scratch is 24 bytes per pool element of ONE column.
 *
 * Every call returns when its results are in the outputs.  Errors (BH_EINVAL, BH_EHIP, BH_ENOMEM) leave their message in
 * bh_engine_last_error.  BH_EINVAL for an argument -- a group value outside [-1, G), an empty group, a zoff that is negative or
 * beyond 2^40, T*C >= 2^32 -- launches nothing; BH_EINVAL for the data (a value of a kept chain that is not finite, a kept model
 * row that is not a row) is found by a first pass over all columns before anything is written.  Neither writes to the outputs.
 */
#ifndef BH_ENGINE_CHAIN_RANK_H
#define BH_ENGINE_CHAIN_RANK_H

#include "bh_engine.h"
#include "bh_engine_chain_diag.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BH_RANK_TILE 4096        /* keys of one workgroup of a sort pass */
#define BH_RANK_RADIXBITS 8      /* bits per pass */

/* memspace, stream, elem_bytes, T, C, Q, ld_t, ld_c, x: as in bh_chain_diag_series (1 <= Q <= BH_DIAG_MAXCOLS).  G >= 1,
 * group: host [C];  zt: host, zoff: host [G] (both may be NULL when z and zf are);  ld_out_c >= Q, ld_out_t >= 1. */
int bh_chain_rank_series(bh_engine *e, int memspace, void *stream, int elem_bytes, int64_t T, int C, int Q, int64_t ld_t,
                         int64_t ld_c, const void *x, int G, const int32_t *group, const double *zt, const int64_t *zoff,
                         double *z, double *zf, float *tail, int64_t ld_out_t, int64_t ld_out_c);

/* The same for the series derived from model rows (bh_chain_diag_models: ML, ld_c >= 2*ML, D <= BH_DIAG_MAXDEPTHS depths dep,
 * host, finite and strictly ascending; column q < D the vs at depth dep[q], column D nlayers): the columns q0 .. q0 + nq - 1 of
 * those D + 1 are ranked (0 <= q0, 1 <= nq, q0 + nq <= D + 1) and are the columns 0 .. nq - 1 of the outputs (ld_out_c >= nq).
 * The values are formed in the kernels from the rows. */
int bh_chain_rank_models(bh_engine *e, int memspace, void *stream, int elem_bytes, int64_t T, int C, int ML, int64_t ld_t,
                         int64_t ld_c, const void *models, int D, const double *dep, int q0, int nq, int G, const int32_t *group,
                         const double *zt, const int64_t *zoff, double *z, double *zf, float *tail, int64_t ld_out_t,
                         int64_t ld_out_c);

#ifdef __cplusplus
}
#endif
#endif
