/*
 * include/bh_engine_ellip_target.h -- the Rayleigh ellipticity (include/bh_engine_swd_ellip.h) as a registered target with a forward
 * model: the fused calls bh_evaluate_batch / bh_evaluate_sites, and with them the device chains, run it.  libbh_engine.so.
 *
 * An extension outside the drop-in contract of include/bh_engine.h, whose ABI version and declarations stay.  A target enters
 * bh_targets_set as a BH_TARGET_USER -- observed data and a noise law -- and bh_targets_set_ellip then gives it a forward model.
 *
 * THE FORWARD MODEL of target t, per model b and period k:
 *     hv = the ellipticity of the fundamental Rayleigh mode at periods[k], from a phase velocity of the engine's search polished
 *          by nsteps secant steps: bh_swd_ellip(have_vel = 1, nsteps) of include/bh_engine_swd_ellip.h
 *     y  = zh ? 1.0 / hv : hv;   if not is_signed: y = fabs(y)
 * written to column off_t + k of the model's row of ymod.
 *
 * A FUSED CALL with such a target.
 *   Failure.  err_t[t][b] != 0 -- hence logL = -1e15, misfits = 1e15, err[b] = 1 -- exactly when the phase-velocity search found
 *     no root for model b (its failure flag), or one of the model's K entries raised the flag of bh_swd_ellip (a water layer, a
 *     polish step that left the window, a vanishing component, a mismatch of the two expressions of hv above
 *     BH_ELLIP_MISMATCH_MAX -- the gate: the fused build forms the mismatch without writing it), or one of its K values y is not
 *     finite (zh at hv == 0 included).  So no synthetic that the arithmetic does not determine reaches the likelihood: about a third
 *     of the (model, period) pairs drawn from a chain's prior fail this way (profiles/swd_ellip_accuracy.txt).
 *   Values.  A lane whose y is not finite writes 0.0; a lane without a root (the search failed, or its velocity is not positive)
 *     writes 0.0, or fails as above where the transform of 0.0 is not finite.  The other ymod columns of a FAILED model are
 *     unspecified (a lane may see its model's failure raised by a neighbour and write 0.0, or may not).
 *   Bits.  For every model that does not fail, the target's columns of ymod are the bits of
 *       1. bh_swd_batch (BH_WAVE_RAYLEIGH, BH_VEL_PHASE, mode 1, flsph 0) at `periods`, with the engine's search, arithmetic and trials,
 *       2. bh_swd_ellip(have_vel = 1, nsteps) on those velocities and failure flags,
 *       3. the transform above,
 *     and logL and misfits are those of bh_loglike_batch on the synthetics so made.
 *
 * ONE SEARCH WHERE ONE SUFFICES.  The ellipticity is almost always inverted beside the Rayleigh phase velocities at the same
 * periods.  The call's plan (bh_plan_ellip below) lets target t READ the velocities of the first registered target j that is a
 * dispersion target of Rayleigh waves, phase velocity, mode 1, flsph 0, run at its own periods (at most 60), whose periods equal
 * `periods` bit for bit -- unless a table of periods per site (bh_sites_set_x ...) is in force, under which target j's periods are
 * its sites' own.  The ellipticity then costs no search: it reads ymod + off_j and takes the search's failures from row j of err_t.
 * Otherwise the call runs a search of its own for target t -- one more job of the call's ONE dispersion launch -- into a
 * workspace.  Under a period table that job reads the table's column of target t like every dispersion job; the column holds the
 * one set of periods all sites share (below).  Two ellipticity targets never share a search with each other: each without a
 * dispersion target to read runs its own, equal periods or not.
 *
 * SITES.  bh_targets_set_ellip belongs between bh_targets_set and any bh_sites_set*.  Every site shares the target's periods: the
 * count tables (bh_sites_set_x ... bh_sites_set_axes) take the descriptor's count for it at every site -- a count of 0, a site
 * that lacks the target, is refused with BH_EUNSUPPORTED -- and x equal to `periods` bit for bit (BH_EINVAL otherwise).
 * (Periods per site and sites without the target: bh_targets_set_ellip_sites of include/bh_engine_sites_ellip.h, opt-in.)
 *
 * bh_loglike_batch serves a target set with such a target as it serves a BH_TARGET_USER: the caller's synthetics.
 */
#ifndef BH_ENGINE_ELLIP_TARGET_H
#define BH_ENGINE_ELLIP_TARGET_H

#include "bh_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BH_TARGET_ELLIP 3 /* the kind of a target after bh_targets_set_ellip, until the next bh_targets_set */

/* Give registered target t the forward model above: K periods [s] (host array, copied), nsteps polish steps, is_signed and zh as
 * in the transform (0 / non-zero).
 * BH_EINVAL with a message, nothing changed: t out of range; the target's kind is not BH_TARGET_USER; K differs from the
 * target's n; K outside 1..60; periods null or a period that is not finite and positive; nsteps outside 0..3; a site table is
 * in force. */
int bh_targets_set_ellip(bh_engine *e, int t, int K, const double *periods, int nsteps, int is_signed, int zh);

/* The plan's decision, pure: no HIP call, no engine; callable on a machine without a GPU.
 * nt registered targets (at most 8); per target kind (BH_TARGET_*), and -- read for the dispersion and ellipticity targets --
 * iwave, igr, mode, flsph, n (the descriptor's count) and xid: an id of the bit pattern of its periods, equal ids for equal bits.
 * x_table != 0: a table of periods per site is in force.
 * source[t] (nt entries): for a BH_TARGET_ELLIP target the index j of the target whose search it shares, or -1 for a search of its
 * own; -2 for every other kind.  Returns the number of searches added to the call's dispersion launch (the -1 entries), or -1
 * for nt outside 0..8 or a null argument. */
typedef struct {
    int32_t kind, iwave, igr, mode, flsph, n, xid;
} bh_ellip_plan_target;
int bh_plan_ellip(int nt, const bh_ellip_plan_target *targets, int x_table, int32_t *source);

#ifdef __cplusplus
}
#endif
#endif
