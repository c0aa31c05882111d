/*
 * include/bh_engine_sites_rf.h -- receiver-function parameters per site of libbh_engine.so.
 *
 * An extension of include/bh_engine_sites.h, outside the drop-in contract of include/bh_engine.h.  With the table of this header
 * the sites of a site table share every receiver-function call argument of the descriptors registered by bh_targets_set but two:
 * the ray parameter p (the slowness of a station's RF stack depends on the events that station recorded) and the near-surface
 * velocity nsv.  Both enter only the frequency-independent coefficients of a model, so one batch may still mix models of many
 * sites.  (The time axis and the Gauss width become a site's own with include/bh_engine_sites_rf_axis.h, which builds on this table.)
 */
#ifndef BH_ENGINE_SITES_RF_H
#define BH_ENGINE_SITES_RF_H

#include "bh_engine_sites.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The ray parameter p_s_per_deg[s*nt + t] (s/deg) and near-surface velocity nsv[s*nt + t] (km/s; <= 0: the model's top-layer
 * vs, as in the descriptor) of site s for target t, nt = the number of targets registered by bh_targets_set.  Column t is
 * read only when target t is a BH_TARGET_RF.  Host arrays [nsites][nt], copied to the device.
 * With the table, bh_evaluate_sites gives model b the p and nsv of site site[b] for every receiver-function target -- the
 * same bits as a call whose descriptor holds those values; the descriptor's Gaussian width, sampling, time shift and length
 * stay shared unless bh_sites_set_rf_axis follows (include/bh_engine_sites_rf_axis.h), the wave type in any case.  Without it (the default) bh_evaluate_sites uses the descriptor's p and nsv.
 * bh_evaluate_batch and bh_rf_batch never read the table.  bh_sites_set and bh_targets_set drop it; another call replaces it
 * and drops the table of bh_sites_set_rf_axis.
 * BH_EINVAL without a site table (bh_sites_set), when nsites differs from the table's, for a NULL array, and when a
 * receiver-function column holds a non-finite value. */
int bh_sites_set_rf(bh_engine *e, int nsites, const double *p_s_per_deg, const double *nsv);

#ifdef __cplusplus
}
#endif
#endif
