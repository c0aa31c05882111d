/*
 * include/bh_engine_sites_x_all.h -- dispersion periods per site on EVERY dispersion target of libbh_engine.so.
 *
 * An extension of include/bh_engine_sites_x.h, outside the drop-in contract of include/bh_engine.h.  bh_sites_set_x serves
 * fundamental-mode phase velocities; group velocities -- what ambient-noise and FTAN processing delivers most often -- and higher
 * modes have their own usable band at every station just as much.  The entry point of this header registers the same table and
 * lets every dispersion target the engine serves differ from site to site in its periods and their count: phase or group
 * velocity, modes 1 to 3, Rayleigh or Love, flat or flattened.  bh_sites_set_x keeps every refusal it has.
 */
#ifndef BH_ENGINE_SITES_X_ALL_H
#define BH_ENGINE_SITES_X_ALL_H

#include "bh_engine_sites_x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bh_sites_set_x without its refusal of per-site periods on group-velocity and higher-mode targets: the same arguments and
 * layout (n[s*nt + t], x / yobs / yerr[s*ldy + off_t + i]; host arrays, copied), the same scaled-error tables (the helper
 * bh_targets_set and bh_sites_set share, over a site's own n) and the same lifetime -- bh_targets_set, bh_sites_set and
 * bh_sites_set_x drop the table, bh_sites_set_rf may follow it, bh_evaluate_batch never reads it.
 * The descriptor n of every dispersion target is the CAPACITY of its ymod columns (at most 60), its x a placeholder that is
 * never read.  bh_evaluate_sites searches model b at the periods of site site[b] and writes its n velocities followed by zeros
 * up to the capacity; the reference's failure convention holds within the first n.  A group velocity split in two launches
 * (the chain of first roots, then one search per second root) finds both at the model's own periods: an entry of the second
 * launch whose period index is at or beyond its site's count does nothing.  A model gets the bits of a one-site call whose
 * descriptors are its site's.  BH_DEVICE: a site index out of range reads nothing of the table and fails in band (err = 1,
 * logL = -1e15, zeros).
 * BH_EINVAL: a NULL n, x or yobs (or yerr with a BH_LAW_NOCORR_SCALED target); a dispersion count below 1 or above the capacity;
 *   a period that is not finite and positive; a dispersion target with the Gauss law (its R^-1 depends on n); another count
 *   than the descriptor's for a target that is no dispersion curve.
 * BH_EUNSUPPORTED (not built): a dispersion target of more than 60 periods (the interpolation path). */
int bh_sites_set_x_all(bh_engine *e, int nsites, const int32_t *n, const double *x, const double *yobs, const double *yerr);

#ifdef __cplusplus
}
#endif
#endif
