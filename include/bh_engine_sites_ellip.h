/*
 * include/bh_engine_sites_ellip.h -- the Rayleigh ellipticity target (include/bh_engine_ellip_target.h) with its own periods at
 * every site, or absent at a site, for libbh_engine.so.
 *
 * An extension of include/bh_engine_ellip_target.h and include/bh_engine_sites_missing.h, outside the drop-in contract of
 * include/bh_engine.h, whose ABI version and declarations stay.  H/V curves come out of noise or earthquake processing station by
 * station: each has its own usable band, rarely the band of the station's phase-velocity curve, and many stations have no usable
 * curve at all.  Without the call of this header a BH_TARGET_ELLIP target keeps every rule of bh_engine_ellip_target.h: one set of
 * periods for all sites, no site without it.
 *
 * THE RULE PER MODEL.  A model of site s gets the logL, misfits, err and synthetics of a one-site fused call
 * (bh_evaluate_batch) whose ellipticity target has site s's periods: its n values, then zeros up to the capacity of the
 * target's columns.  For a site that lacks the target the rule of include/bh_engine_sites_missing.h holds: nothing is added to
 * logL, the target's misfit is 0, it never sets err, its columns are zero, its forward model is not run.  BH_DEVICE: a site index
 * out of range reads nothing of the table and fails in band, as before.
 *
 * ONE SEARCH WHERE ONE SUFFICES, per site.  bh_plan_ellip_sites below decides once, when the count table is registered, whether
 * such a target reads the velocities of a dispersion target of the call or runs a search of its own (one more job of the call's
 * one dispersion launch, at the table's column of the target).  The decision is kept with the site table; the fused call reads it.
 */
#ifndef BH_ENGINE_SITES_ELLIP_H
#define BH_ENGINE_SITES_ELLIP_H

#include "bh_engine_ellip_target.h"
#include "bh_engine_sites_missing.h"

#ifdef __cplusplus
extern "C" {
#endif

/* own != 0: target t, a BH_TARGET_ELLIP, takes its periods and their count from the count table, site by site.  Called between
 * bh_targets_set_ellip and any bh_sites_set*.  The periods registered by bh_targets_set_ellip are then a placeholder that is
 * never read, and the target's n is the CAPACITY of its ymod columns (at most 60), exactly as for a dispersion target under
 * bh_sites_set_x_all.  own == 0 takes the flag back; bh_targets_set resets it.
 * For such a target the count tables apply the rules of a dispersion target: a count of 1 .. capacity, a count of 0 -- the site
 * lacks the target -- from bh_sites_set_missing on, every period finite and positive, the Gauss law refused.  bh_sites_set and
 * bh_sites_set_x refuse the target by name (BH_EINVAL): it needs the table of bh_sites_set_x_all or of a later entry point.
 * bh_evaluate_batch, which reads no table, refuses a target set that holds such a target (BH_EINVAL).
 * BH_EINVAL with a message, nothing changed: t out of range; the target's kind is not BH_TARGET_ELLIP; a site table is in
 * force. */
int bh_targets_set_ellip_sites(bh_engine *e, int t, int own);

/* The plan's decision under a count table, pure: no HIP call, no engine; callable on a machine without a GPU.
 * nt registered targets (at most 8) as bh_plan_ellip reads them (xid is not read: the periods are the table's); own[nt]: the flag
 * above per target; the host tables of nsites sites: n[s * nt + t] counts, x[s * ldx + off[t] + i] periods, off[nt] the
 * targets' column offsets.
 * source[t] (nt entries): -2 for a target that is no BH_TARGET_ELLIP.  For a flagged ellipticity target t the first target j that
 * is a dispersion target of Rayleigh waves, phase velocity, mode 1, flsph 0 with a capacity of at most 60 such that AT EVERY SITE
 * THAT HAS t (count > 0) site s has j with the same count and bit-identical periods; -1, a search of its own, if there is none.
 * A site that has j and lacks t does not matter; a site that has t and lacks j forces the search.  An ellipticity target without
 * the flag gives -1 under a table, as bh_plan_ellip does.  Two ellipticity targets never share a search with each other.
 * Returns the number of searches added to the call's dispersion launch (the -1 entries), or -1 for nt outside 0..8, nsites < 1
 * or a null argument. */
int bh_plan_ellip_sites(int nt, const bh_ellip_plan_target *targets, const int32_t *own, int nsites, const int32_t *n,
                        const double *x, int ldx, const int32_t *off, int32_t *source);

#ifdef __cplusplus
}
#endif
#endif
