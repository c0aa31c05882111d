/*
 * include/bh_engine_sites_x.h -- dispersion periods per site of libbh_engine.so.
 *
 * An extension of include/bh_engine_sites.h, outside the drop-in contract of include/bh_engine.h.  Stations of an array rarely
 * share the periods of their dispersion curves: every curve has its own usable band, and quality control drops periods station
 * by station.  surfdisp96 starts the search at period k from the root at period k - 1, so a curve on a subset of the periods is
 * not the same curve, and a site's models have to be computed at that site's own periods, with the searches a one-site call
 * makes.  With the table of this header a batch still mixes models of many sites: every model's dispersion curves are computed
 * at its own site's periods and its likelihood runs over its own site's sample counts -- the bits of a one-site call.
 */
#ifndef BH_ENGINE_SITES_X_H
#define BH_ENGINE_SITES_X_H

#include "bh_engine_sites.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The site table (as bh_sites_set) together with every site's periods: a sibling of bh_sites_set, not an add-on to it, because
 * the scaled-error law's yerr / min(yerr) and ln prod run over a site's own samples.
 *   n[s*nt + t]            samples of site s for target t (nt = the targets registered by bh_targets_set)
 *   x[s*ldy + off_t + i]   period i of site s for dispersion target t, in ymod's column layout (ldy = sum_t n_t of the
 *                          descriptors); yobs and yerr likewise (yerr: BH_LAW_NOCORR_SCALED targets only, NULL if there is none)
 * Columns i >= n[s*nt + t] are not read.  Host arrays, copied.
 * bh_targets_set registers the structure as always; a dispersion target's descriptor n is the CAPACITY of its ymod columns
 * (the largest count of any site, at most 60) and its descriptor x a placeholder that bh_evaluate_sites does not read.  For a
 * target that is no dispersion curve n[s*nt + t] must equal the descriptor's n, and x is not read.
 * With the table, bh_evaluate_sites (unchanged in signature) searches model b at the periods of site site[b] -- the site-period
 * builds of the dispersion kernels -- and writes, in a dispersion target's ymod columns, its n velocities followed by zeros up
 * to the capacity; the reference's failure convention holds within the first n (err = 1, zeros from the failing period on).
 * logL and misfits run over the site's n samples.  BH_DEVICE: a site index out of range reads nothing of the table and fails
 * in band.  The scaled-error tables come from the helper bh_targets_set and bh_sites_set share: the bits of a one-site
 * registration with the site's own n.
 * bh_evaluate_batch never reads the table.  bh_targets_set and bh_sites_set drop it; bh_sites_set_rf may follow it (the two
 * are independent and work together).
 * BH_EINVAL: a NULL n, x or yobs (or yerr with a BH_LAW_NOCORR_SCALED target); a dispersion count below 1 or above the capacity;
 *   a period that is not finite and positive; a dispersion target with the Gauss law (its R^-1 depends on n); another count
 *   than the descriptor's for a target that is no dispersion curve.
 * BH_EUNSUPPORTED (not built): a group-velocity or higher-mode target whose periods or count differ from its descriptor's at
 *   some site (sites that share the descriptor's periods on such targets are fine); a dispersion target of more than 60 periods
 *   (the interpolation path).  Receiver functions keep one x (per-site p / nsv: bh_engine_sites_rf.h). */
int bh_sites_set_x(bh_engine *e, int nsites, const int32_t *n, const double *x, const double *yobs, const double *yerr);

#ifdef __cplusplus
}
#endif
#endif
