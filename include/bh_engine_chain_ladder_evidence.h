/*
 * include/bh_engine_chain_ladder_evidence.h -- the rung series of tempered runs and the sums of their evidence estimates:
 * libbh_engine.so.
 *
 * An extension like include/bh_engine_chain_diag_ladders.h, outside the drop-in contract of include/bh_engine.h.  A tempering ladder
 * samples prior x L^beta at every one of its betas; the ratios Z(b_{r-1}) / Z(b_r) of neighbouring rungs, and with them the log
 * marginal likelihood, are estimated from the log-likelihoods recorded on the rungs (stepping stones, thermodynamic integration:
 * bayhunter_amd/diagnostics.py, ladder_evidence).  No chain's recorded series is a rung's series: the betas move between the chains.
 * This header finds the chain that holds every rung at every row, and forms the sums over every rung's series, from the tables
 * where record="device" wrote them.
 *
 * Inputs: beta[t*ld_t + c] (float64) and the recorded log-likelihoods x[t*ldx_t + c*ldx_c] (elem_bytes 4 or 8, converted to float64
 * on read), t < T rows, c < C chains; ladder[c] in 0..K-1, R the size of the largest ladder -- as in bh_chain_ladder_index.
 * Series are numbered as the members are: ladder k of R_k chains owns the series j = start[k] + r, r < R_k, rung 0 cold; start is
 * the prefix sum of the ladder sizes in ascending id (what diagnostics.ladder_index returns as members, concatenated).
 *   hold[t][j]   = the chain c of ladder k with rung[t][c] == r, rung as in include/bh_engine_chain_diag_ladders.h
 *   b_j          = the beta held at series j: the same bits at every row; rung_beta[j], descending within a ladder
 *   l_j[t]       = (double)x[t][hold[t][j]]
 *   mx_j, mn_j   = max_t l_j[t], min_t l_j[t]                                            exact, independent of any order
 *   Df_j         = fl(b_{j-1} - b_j) for r >= 1, 0 for r = 0                            the step to the colder rung
 *   Dr_j         = fl(b_j - b_{j+1}) for r <= R_k - 2, 0 on the hottest rung            the step to the hotter rung
 *   af           = fl(Df_j * fl(l - mx_j)),   wf = exp(af)
 *   ar           = fl(-Dr_j * fl(l - mn_j)),  wr = exp(ar)
 *   exp          : glibc's bits (bayhunter_amd/csrc/bh_libm.h: the table path for 2^-54 <= |a| < 512, 1 + a below 2^-54); a term
 *                  with a <= -512 is exactly 0 and reaches no other exp
 *   Sf = sum_t wf,  Sf2 = sum_t fl(wf * wf),  Sr = sum_t wr,  Sr2 = sum_t fl(wr * wr)
 * Every sum in the 16 strands of include/bh_engine_chain_diag.h: strand s adds the rows t = s (mod 16) in ascending t, starting
 * from 0, and the strands are combined in that header's tree.  No product is contracted into a sum (-ffp-contract=off).  A series
 * with a step of 0 returns exactly T and T.  The order depends on T only: a ladder's numbers are the same bits alone or among other
 * ladders, with its chains in any column order, from host or device memory, with any leading dimensions, and on every repeat.
 * Elements of x and beta between the strides are never read.
 *
 * Every call returns when its results are in host memory (hold of a BH_DEVICE call: when it is written).  Errors leave their message
 * in bh_engine_last_error and write nothing to any output:
 *   BH_EINVAL       an argument (nothing is launched); the data, found by the first passes: a beta or a like that is not finite,
 *                   two equal betas in one ladder at some row ("tied betas": a rung would have two holders), a rung whose beta
 *                   changes between rows ("the betas of a ladder change within the rows": a burn-in phase in which the ladder
 *                   adaptation moved them)
 *   BH_EUNSUPPORTED a ladder of more than BH_LADDER_MAXRUNGS chains
 */
#ifndef BH_ENGINE_CHAIN_LADDER_EVIDENCE_H
#define BH_ENGINE_CHAIN_LADDER_EVIDENCE_H

#include "bh_engine_chain_diag_ladders.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BH_EVIDENCE_DROP 512     /* a term exp(a) with a <= -BH_EVIDENCE_DROP is exactly 0 */

/* beta, ladder, K, R, memspace and stream: as in bh_chain_ladder_index.  hold: int32 [T][C] with row stride ld_hold >= C, in memspace
 * -- a valid sel of the bh_chain_diag_*_sel calls with K = C series.  rung_beta: host [C]. */
int bh_chain_ladder_holders(bh_engine *e, int memspace, void *stream, int64_t T, int C, int64_t ld_t, const double *beta,
                            const int32_t *ladder, int K, int R, int32_t *hold, int64_t ld_hold, double *rung_beta);

/* ... and the sums.  x: the likes in memspace, ldx_t >= 1, ldx_c >= 1 (elements; no two chains may share an element).  hold may be
 * NULL when only the sums are wanted.  rung_beta, mx, mn, sf, sf2, sr, sr2: host [C], all must be given. */
int bh_chain_ladder_evidence(bh_engine *e, int memspace, void *stream, int64_t T, int C, int64_t ld_t, const double *beta,
                             int elem_bytes, int64_t ldx_t, int64_t ldx_c, const void *x, const int32_t *ladder, int K, int R,
                             int32_t *hold, int64_t ld_hold, double *rung_beta, double *mx, double *mn, double *sf, double *sf2,
                             double *sr, double *sr2);

#ifdef __cplusplus
}
#endif
#endif
