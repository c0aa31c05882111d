/*
 * include/bh_engine_sites_laws.h -- sites with their OWN noise law, for libbh_engine.so.
 *
 * An extension of include/bh_engine_sites_gauss.h (and of include/bh_engine_sites_rf_axis.h, whose count table it accepts as well),
 * outside the drop-in contract of include/bh_engine.h.  A target's noise law is a field of its descriptor (bh_target_desc::law),
 * and every site of the table shared it.  The sampler installs a target's law from the station's own priors and data: a
 * correlation fixed at 0 gives BH_LAW_NOCORR without error bars and BH_LAW_NOCORR_SCALED with them, a receiver function with a
 * fixed non-zero correlation BH_LAW_GAUSS, anything else BH_LAW_EXP.  Stations with their own priors therefore differ in their
 * laws.  The entry point of this header gives every (site, target) pair its own law.
 *
 * The rule: a model of site s gets, on every target, the logL contribution, misfit, joint misfit and failure handling of a call
 * over the same batch (same B, same capacities) in which every site has site s's laws -- bit for bit.  The likelihood's sums are
 * formed in one order whatever the law, and the law only selects among them.  A forward model is run by count, not by law.
 *
 * The descriptor's law keeps two roles: it decides the launch form, and a BH_LAW_GAUSS descriptor owns the contraction's shape and
 * workspace -- so BH_LAW_GAUSS may stand in the table only on a target whose descriptor is under BH_LAW_GAUSS.  The contraction
 * needs no build of its own: the rows of a site that is not under the Gauss law on such a target are in class -1 of the target's
 * class table, belong to no tile, and their slab sums are never read.
 */
#ifndef BH_ENGINE_SITES_LAWS_H
#define BH_ENGINE_SITES_LAWS_H

#include "bh_engine_sites_gauss.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The noise law law[s*nt + t] (int32: BH_LAW_NOCORR .. BH_LAW_GAUSS) of site s on target t, nt = the number of targets registered
 * by bh_targets_set, for the count table in force; yerr[nsites][ldy], every site's errors in ymod's column layout (the layout of
 * the count table's yerr), read over a site's own samples in the columns of the pairs under BH_LAW_NOCORR_SCALED only -- NULL where
 * the table has no such pair.  Host arrays, copied.  An entry where the site's count is 0 is not read.  For every pair under
 * BH_LAW_NOCORR_SCALED the scaled errors yerr / min(yerr) and ln prod of them are formed over the site's own count, whatever the
 * descriptor's law.  bh_evaluate_sites then evaluates every model under its own site's laws (the likelihood builds of
 * like_kernel_l.hip).  bh_evaluate_batch and bh_loglike_batch never read the table; without it every call behaves as before.
 * Order: after the count table (the one that accepts a Gauss-law target some site lacks, include/bh_engine_sites_gauss.h, or the
 *   one of include/bh_engine_sites_rf_axis.h) and the receiver-function tables, BEFORE the class tables of a Gauss-law target.
 * With the table in force the class-table call of include/bh_engine_sites_gauss.h accepts class -1 exactly where the count is 0 or
 *   the site's law on that target is not BH_LAW_GAUSS, and demands a class >= 0 where it is BH_LAW_GAUSS.  A BH_LAW_GAUSS descriptor
 *   with a present site under another law NEEDS its class table: until it is registered bh_evaluate_sites returns BH_EINVAL with a
 *   message that names bh_sites_set_gauss.  With BH_NO_MFMA (the in-kernel mat-vec) a site under another law reads no matrix.
 * Lifetime: bh_targets_set and every bh_sites_set* entry point that registers or extends the site table (the count tables, the
 *   receiver-function tables) drop the law table; this call drops the class tables of all targets; another call replaces the table.
 * BH_EINVAL: no site table; no count table of the two kinds named above; nsites differs from the table's; law NULL; for a present
 *   pair a law outside BH_LAW_NOCORR .. BH_LAW_GAUSS, BH_LAW_GAUSS on a target whose descriptor is not BH_LAW_GAUSS, or
 *   BH_LAW_NOCORR_SCALED with yerr NULL or with an error that is not finite and positive inside the site's count.
 * BH_EUNSUPPORTED: none. */
int bh_sites_set_laws(bh_engine *e, int nsites, const int32_t *law, const double *yerr);

#ifdef __cplusplus
}
#endif
#endif
