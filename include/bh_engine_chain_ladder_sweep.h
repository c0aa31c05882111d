/*
 * include/bh_engine_chain_ladder_sweep.h -- the swap sweep of tempered chains as one kernel: libbh_engine.so.
 *
 * An extension outside the drop-in contract of include/bh_engine.h.  A tempered run exchanges the temperatures of neighbouring
 * rungs of every ladder; this header does one such sweep of all ladders in one launch, counts what it proposed and accepted per
 * neighbouring pair of rungs, and -- during burn-in, on request -- moves the interior temperatures of a ladder so that its pairs
 * accept at equal rates.  A plan holds the ladders' member lists and every counter on the device.
 *
 * Layout.  ladder[c] in 0..K-1 is chain c's ladder; ladder k has R_k chains, start[k] = R_0 + .. + R_(k-1).  Position start[k] + r
 * is rung r of ladder k (rung 0 the coldest) and, for a counter, the pair (r, r+1); position start[k] + R_k - 1 of a counter is
 * never written.  logu and the rung betas are in this layout.
 *
 * One sweep of ladder k with R chains (all in float64, no product and sum contracted, a comparison with a NaN is false):
 *  1. order = the ladder's chains sorted by (beta descending, chain index ascending); b[r] = beta[order[r]], l[r] = like[order[r]].
 *  2. for r = parity, parity+2, .. with r+1 < R: proposed[phase][r] += 1, wprop[r] += 1; the pair is accepted iff
 *         logu[r] < (b[r] - b[r+1]) * (l[r+1] - l[r])
 *     and then chain order[r] takes b[r+1] (it now holds rung r+1), chain order[r+1] takes b[r] (it holds rung r),
 *     accepted[phase][r] += 1, wacc[r] += 1.  A chain of no accepted pair keeps its beta and its rung.
 *  3. only if adapt != 0 and R >= 3:
 *     if some wprop[i] == 0 (i < R-1): skipped += 1, the betas stay;
 *     else  A[i]  = (double)wacc[i] / (double)wprop[i]
 *           Abar  = (A[0] + A[1] + ..) / (R-1)                       summed in ascending i
 *           g[i]  = b[i] - b[i+1],  span = b[0] - b[R-1],  f = 0x1p-20 * span
 *           x[i]  = g[i] * (1.0 + kappa * (A[i] - Abar)),  g1[i] = x[i] > f ? x[i] : f
 *           s     = g1[0] + g1[1] + ..                               summed in ascending i
 *           g2[i] = (g1[i] * span) / s
 *           nb[0] = b[0],  nb[r] = nb[r-1] - g2[r-1] for r = 1..R-2,  nb[R-1] = b[R-1]
 *           if nb[r] > nb[r+1] for every r < R-1: the chain that holds rung r after step 2 gets nb[r], adaptations += 1;
 *           else skipped += 1, the betas stay.
 *     In both cases wprop and wacc of the ladder are set to 0.  A ladder of 1 or 2 chains never adapts and counts neither.
 *  The rung betas of the plan are then the ladder's betas in descending order: nb after an adaptation, else b.
 *
 * The ends of a ladder never change: nb[0] and nb[R-1] are b[0] and b[R-1] bit for bit.  With adapt == 0 the betas are those of
 * bayhunter_amd.parallel.ladder_swap_betas.  tests/ladder_sweep_ref.py restates all of this in numpy; the kernel returns its bits.
 *
 * Errors leave their message in bh_engine_last_error.  BH_EINVAL / BH_EUNSUPPORTED launch nothing and write nothing to the outputs.
 */
#ifndef BH_ENGINE_CHAIN_LADDER_SWEEP_H
#define BH_ENGINE_CHAIN_LADDER_SWEEP_H

#include "bh_engine_chain_diag_ladders.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bh_ladder_sweep bh_ladder_sweep;

/* ladder: host int32 [C], values 0..K-1, every id used (else BH_EINVAL); a ladder of more than BH_LADDER_MAXRUNGS chains is
 * BH_EUNSUPPORTED.  Every counter of the new plan is 0.  *plan is written on success only. */
int bh_ladder_sweep_create(bh_engine *e, int C, const int32_t *ladder, int K, bh_ladder_sweep **plan);

/* One sweep, enqueued on stream (NULL: the engine's); it does not synchronise.  like, logu: device float64 [C], read; beta: device
 * float64 [C], updated in place.  parity, phase: 0 or 1.  adapt != 0 with phase == 1 is BH_EINVAL: the temperatures of the main
 * phase are frozen. */
int bh_ladder_sweep_run(bh_engine *e, bh_ladder_sweep *plan, void *stream, const double *like, double *beta, const double *logu,
                        int parity, int phase, int adapt, double kappa);

/* Waits for the stream of the plan's last sweep and copies out, to host memory: proposed, accepted: int64 [2][C] (phase, position);
 * rung_beta: float64 [C] as the last sweep left them (0 before the first); adaptations, skipped: int64 [K].  Any may be NULL. */
int bh_ladder_sweep_read(bh_engine *e, bh_ladder_sweep *plan, int64_t *proposed, int64_t *accepted, double *rung_beta,
                         int64_t *adaptations, int64_t *skipped);

/* Waits for the plan's last sweep and frees the plan (NULL: nothing). */
int bh_ladder_sweep_destroy(bh_engine *e, bh_ladder_sweep *plan);

#ifdef __cplusplus
}
#endif
#endif
