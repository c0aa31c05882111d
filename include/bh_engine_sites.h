/*
 * include/bh_engine_sites.h -- many stations at once: site-indexed likelihood of libbh_engine.so.
 *
 * An extension of include/bh_engine.h, outside its drop-in contract.  A SITE is one station's observed data for the target
 * structure registered by bh_targets_set: the same targets, the same x, the same noise laws (for the Gauss law the same R^-1),
 * only the observed values y -- and, for BH_LAW_NOCORR_SCALED targets, yerr -- differ.  The forward models depend on the
 * model and x only, so one batch may mix models of many sites: each is compared with the observed data of its own.
 */
#ifndef BH_ENGINE_SITES_H
#define BH_ENGINE_SITES_H

#include "bh_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Observed data of S sites for the targets registered by bh_targets_set (same targets, same x, same laws):
 * yobs[s*ldy + off_t + i] (ldy = sum_t n_t, target after target, as ymod); yerr likewise, read for
 * BH_LAW_NOCORR_SCALED targets only (NULL if there is none).  Host pointers, copied.  The per-site
 * yerr/min(yerr) and ln prod are formed by the same host code bh_targets_set uses (one helper, same bits).
 * bh_targets_set drops the site table. */
int bh_sites_set(bh_engine *e, int nsites, const double *yobs, const double *yerr);

/* bh_evaluate_batch with site[b] in [0, nsites) selecting the observed data model b is compared with
 * (the caller's order of models; the engine's internal depth sort does not change it).
 * BH_HOST: site indices are checked on the host (BH_EINVAL before anything is launched).  BH_DEVICE: a model whose site index
 * is out of range reads no observed data and is reported failed in band (err 1, logL -1e15, misfits 1e15).
 * BH_EINVAL without a site table (bh_sites_set) and for BH_TARGET_USER targets, as bh_evaluate_batch.
 * Receiver functions write their traces to the ymod workspace on this path (no fused likelihood sums): the likelihood
 * kernel forms the sums, in the same order -- the same bits. */
int bh_evaluate_sites(bh_engine *e, int memspace, void *stream, int B, int Lmax, const int32_t *nlay,
                      const double *h, const double *vp, const double *vs, const double *rho,
                      ptrdiff_t stride_l, ptrdiff_t stride_b, const int32_t *site, const double *noise,
                      double *logL, double *misfits, int32_t *err, double *ymod);

#ifdef __cplusplus
}
#endif
#endif
