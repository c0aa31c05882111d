/*
 * include/bh_engine_chain_diag_ladders.h -- the chain diagnostics of tempered runs: libbh_engine.so.
 *
 * An extension of include/bh_engine_chain_diag.h, outside the drop-in contract of include/bh_engine.h.  In a tempered run the
 * posterior series of a ladder is its cold series: at row t the state of whichever chain of the ladder holds the largest beta.
 * No chain's own recorded series is one.  This header
 *   - finds that chain per (row, ladder) from the recorded table of betas, with the numbers that say whether the ladder mixes
 *     (bh_chain_ladder_index), and
 *   - forms the sums and medians of include/bh_engine_chain_diag.h for series that read another chain at every row
 *     (bh_chain_diag_*_sel), from the tables where record="device" wrote them: nothing is gathered or copied.
 *
 * Definitions, all in integers.  beta[t*ld_t + c], t < T rows, c < C chains; ladder[c] in 0..K-1 is c's ladder, M(c) the chains of
 * c's ladder, R the size of the largest ladder.
 *   rung[t][c]      = #{c' in M(c) : beta[t][c'] > beta[t][c]}            rung 0 is cold; ties share a rung
 *   sel[t][k]       = min{c in ladder k : rung[t][c] == 0}                the first of the largest beta
 *   c is hot at t     when no chain of M(c) has a smaller beta and rung[t][c] > 0
 *   occupancy[c][r] = #{t : rung[t][c] == r},  r < R
 *   round_trips[c]  : walk t ascending with a state in {none, cold seen, hot seen after cold}; a cold row in the third state
 *                     counts one trip; every cold row sets "cold seen"; a hot row in "cold seen" sets the third state
 *   moves[k]        = #{t >= 1 : sel[t][k] != sel[t-1][k]}
 *
 * The gathered calls: series (k, q) reads chain sel[t*ld_sel + k] at row t.  Every output has the bits that the call of
 * include/bh_engine_chain_diag.h returns for the table gathered on the host, x'[t][k][q] = x[t][sel[t][k]][q]: the same strands,
 * the same tree, the same ring, no contraction -- the order of every sum depends on (T, L) only.  An index is checked before it
 * is used as an address (it is clamped for the read and flagged); elements of chains not selected at a row are never read.
 *
 * Every call returns when its results are in host memory (sel and rung of a BH_DEVICE call: when they are written).  Errors leave
 * their message in bh_engine_last_error.  BH_EINVAL / BH_EUNSUPPORTED for an argument launches nothing; BH_EINVAL for the data
 * (a beta or value that is not finite, a model row that is not a row, an index outside [0, C)) is found by the first pass.
 * Neither writes anything to the outputs.
 */
#ifndef BH_ENGINE_CHAIN_DIAG_LADDERS_H
#define BH_ENGINE_CHAIN_DIAG_LADDERS_H

#include "bh_engine_chain_diag.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BH_LADDER_MAXRUNGS 64    /* chains of one ladder */

/* beta: float64 [T][C] with row stride ld_t >= C (elements), in memspace (BH_HOST: copied to the device; BH_DEVICE: read where it
 * lies on stream, NULL: the engine's).  ladder: host int32 [C], values 0..K-1, every id used (else BH_EINVAL); a ladder of more
 * than BH_LADDER_MAXRUNGS chains is BH_EUNSUPPORTED.  R: the size of the largest ladder (BH_EINVAL if it is not).
 * sel: int32 [T][K] with row stride ld_sel >= K, and rung (may be NULL): int32 [T][C] with row stride ld_rung >= C, both in
 * memspace.  occupancy [C][R], round_trips [C], moves [K]: host int64.  A beta that is not finite is BH_EINVAL. */
int bh_chain_ladder_index(bh_engine *e, int memspace, void *stream, int64_t T, int C, int64_t ld_t, const double *beta,
                          const int32_t *ladder, int K, int R, int32_t *sel, int64_t ld_sel, int32_t *rung, int64_t ld_rung,
                          int64_t *occupancy, int64_t *round_trips, int64_t *moves);

/* bh_chain_diag_series / _models / _medians for K >= 1 series that read chain sel[t*ld_sel + k] (int32, ld_sel >= K, in the
 * memspace of x) of the table x[t*ld_t + c*ld_c + ..], c < C, at row t.  Every other argument as there; the outputs are host
 * [K][Q], [K][Q][L+1] and (medians) [K].  An index outside [0, C) is BH_EINVAL ("index"). */
int bh_chain_diag_series_sel(bh_engine *e, int memspace, void *stream, int elem_bytes, int64_t T, int C, int Q, int64_t ld_t,
                             int64_t ld_c, const void *x, int K, const int32_t *sel, int64_t ld_sel, int L, double *x0, double *s1,
                             double *s1a, double *s1b, double *m2a, double *m2b, double *p);

int bh_chain_diag_models_sel(bh_engine *e, int memspace, void *stream, int elem_bytes, int64_t T, int C, int ML, int64_t ld_t,
                             int64_t ld_c, const void *models, int K, const int32_t *sel, int64_t ld_sel, int D, const double *dep,
                             int L, double *x0, double *s1, double *s1a, double *s1b, double *m2a, double *m2b, double *p);

int bh_chain_diag_medians_sel(bh_engine *e, int memspace, void *stream, int elem_bytes, int64_t T, int C, int64_t ld_t,
                              int64_t ld_c, const void *x, int K, const int32_t *sel, int64_t ld_sel, double *lo, double *hi);

#ifdef __cplusplus
}
#endif
#endif
