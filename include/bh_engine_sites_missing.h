/*
 * include/bh_engine_sites_missing.h -- sites that LACK some of the array's targets, for libbh_engine.so.
 *
 * An extension of include/bh_engine_sites_x_all.h, outside the drop-in contract of include/bh_engine.h.  The site tables so far
 * want every site to have every registered target.  Real arrays do not: a third of the stations may have no usable Love curve,
 * temporary stations too few events for a receiver function, one permanent station an S receiver function nobody else has.  The
 * entry points of this header let the count n[site][target] of the table be ZERO: that site has no such target.
 *
 * The rule: a model of site s gets the logL, the misfits, err and the synthetics of a one-site call whose descriptors are the
 * targets site s HAS, in their order.  For a target the site lacks
 *   - nothing is added to logL and to the joint misfit; its own misfit entry is 0;
 *   - it never sets err: its forward model is not run, and the likelihood does not read its row of the per-target failure flags.
 *     (That row may still hold 1 for such a pair -- the dispersion kernels flag a model with absurd values whatever the count --
 *     so the per-target flags seen through the debug interface are not the rule; err of bh_evaluate_sites is.)
 *   - its ymod columns hold zeros;
 *   - its two noise parameters are never read by the likelihood and -- chains, below -- never proposed or checked.
 * A registered target is a SLOT here: slot i has one class, one descriptor and one noise law wherever it is present.
 */
#ifndef BH_ENGINE_SITES_MISSING_H
#define BH_ENGINE_SITES_MISSING_H

#include "bh_engine_sites_x_all.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bh_sites_set_x_all with a count of 0 allowed on ANY target: the same arguments and layout (n[s*nt + t], x / yobs /
 * yerr[s*ldy + off_t + i]; host arrays, copied; the columns of an absent (site, target) are placeholders, never read), the same
 * helper, the same lifetime.  A dispersion target's count is 0 or 1 .. capacity; a receiver function's is 0 or its descriptor's.
 * bh_evaluate_sites then serves the rule above:
 *   - dispersion (every kernel family of the site-period builds): a (model, target) pair of count 0 makes no secular evaluation,
 *     writes its zero columns, is never listed for the guard's re-run; the entries of a second-root launch are idle;
 *   - receiver functions: the coefficient stage marks the record of such a model absent (distinct from bad) and the workgroup of
 *     the synthesis kernel that finds the mark writes zeros and leaves -- no reflectivity recursion, no inverse transform.  The
 *     coefficient stage needs the model's site: with a receiver-function target registered, bh_sites_set_rf must follow this call
 *     (its p / nsv of an absent (site, target) are not used), else bh_evaluate_sites returns BH_EINVAL;
 *   - likelihood: the target is skipped; the sums are those of the present targets, formed in their order (the bits of the
 *     one-site call).
 * BH_DEVICE: a site index out of range reads nothing of the table and fails in band, as before.
 * BH_EINVAL: what bh_sites_set_x_all refuses, but for a count of 0; a site with no target (every count 0); a target no site has;
 *   a receiver function's count that is neither 0 nor its descriptor's.
 * BH_EUNSUPPORTED: a Gauss-law target some site lacks (the MFMA contraction gathers the sites' rows; skipping rows there is not
 *   built); more than 60 periods, as before.
 * bh_sites_set_x and bh_sites_set_x_all keep refusing a count below 1. */
int bh_sites_set_missing(bh_engine *e, int nsites, const int32_t *n, const double *x, const double *yobs, const double *yerr);

/* bh_chain_propose / bh_chain_propose_window for chains whose sites lack targets: beside their arguments absent[C] (device,
 * one byte per chain), bit t set = the chain's site lacks target t (BH_MAX_TARGETS = 8 bits).  Noise parameter i is FREE iff
 * cfg->noise_lo[i] != cfg->noise_hi[i] AND bit i/2 of the chain's mask is clear: the number of free parameters, whether a noise
 * move is among the chain's moves, the ordinal map from the draw to the parameter and the bounds check all follow that
 * definition.  The random streams do not depend on the number of targets, so a chain whose site has the same free parameters in
 * the same order as a one-site job draws that job's moves and parameters.  The noise entries of an absent target are carried
 * along unchanged.  bh_chain_accept / bh_chain_accept_window serve these chains as they are (they copy noise and misfits, no
 * more).  BH_EINVAL: what the plain entry points refuse; a null mask.  (With the plain entry points, these now refuse a negative
 * cfg->nt or cfg->maxlayers as well -- bh_engine.h; before, only values above the limits.) */
int bh_chain_propose_sites(void *stream, const bh_chain_config *cfg, const bh_chain_state *state, int C, int iiter,
                           const uint8_t *absent);
int bh_chain_propose_window_sites(void *stream, const bh_chain_config *cfg, const bh_chain_state *state, int C, int iiter,
                                  int depth, ptrdiff_t ld, const uint8_t *absent);

#ifdef __cplusplus
}
#endif
#endif
