/*
 * include/bh_engine_sites_rf_axis.h -- sites with their OWN receiver-function time axis and Gauss filter, for libbh_engine.so.
 *
 * An extension of include/bh_engine_sites_rf.h and include/bh_engine_sites_gauss.h, outside the drop-in contract of
 * include/bh_engine.h.  Stations of an array are processed with different windows (-5 .. 20 s at one, -10 .. 40 s at another),
 * different sampling (5, 10, 20 Hz) and different Gauss widths (1.0 against 2.5).  The entry points of this header let the sample
 * count n, the transform length nsamp, the sampling rate fsamp, the time shift tshift and the filter width gauss of a
 * receiver-function target differ from site to site.
 *
 * The rule: a model of site s gets, on a receiver-function target, the trace, the failure behaviour, logL and the misfits of a
 * one-site call whose descriptor holds site s's nsamp, fsamp, tshift, gauss and n (p and nsv: bh_sites_set_rf, as before).  The
 * trace is that call's bit for bit over the site's own n samples and is followed by zeros up to the capacity of the target's
 * ymod columns, the descriptor's n.  The wave type stays a property of the target.  The descriptor's own nsamp, fsamp, tshift and
 * gauss are placeholders on this path: bh_evaluate_sites never reads them.
 *
 * One workgroup of the synthesis kernel is one model, and it reads its site's values where the shared-axis build reads the
 * launch's.  Every workgroup of a launch holds the LDS of the longest trace of the table, so short traces run at the long ones'
 * occupancy.
 */
#ifndef BH_ENGINE_SITES_RF_AXIS_H
#define BH_ENGINE_SITES_RF_AXIS_H

#include "bh_engine_sites_rf.h"
#include "bh_engine_sites_gauss.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The longest transform of a site's record: the trace one workgroup's LDS holds.  (The descriptors' HBM-workspace path for longer
 * traces stays on the shared axis.) */
#define BH_SITES_RF_AXIS_MAX_NSAMP 16384

/* bh_sites_set_missing_gauss that accepts, on a receiver-function target, a count of 0 or 1 .. the descriptor's n: the same
 * arguments, layout, checks but that one, and lifetime.  The descriptor's n is the capacity of the target's ymod columns; yobs
 * (and yerr) beyond a site's count are not read, the table holds zeros there.  A receiver-function count that differs from the
 * descriptor's then NEEDS the table of bh_sites_set_rf_axis: until it is registered bh_evaluate_sites returns BH_EINVAL with a
 * message that names bh_sites_set_rf_axis.  Under the Gauss law such a target needs its class table as well (bh_sites_set_gauss:
 * every site's n x n matrix in the top-left corner of a zero matrix of the capacity, its own ln|R| in logdet_r), and the
 * BH_NO_MFMA in-kernel mat-vec is refused for it (BH_EUNSUPPORTED: its row stride is the site's n, the padded matrix has the
 * capacity's).  bh_sites_set_x, _x_all, _missing and _missing_gauss keep refusing a receiver-function count that is neither the
 * descriptor's nor (the last two) 0. */
int bh_sites_set_axes(bh_engine *e, int nsites, const int32_t *n, const double *x, const double *yobs, const double *yerr);

/* The transform length nsamp[s*nt + t] (int32) and the sampling rate fsamp (Hz), time shift tshift (s) and Gauss width gauss
 * [s*nt + t] of site s for target t, nt = the number of targets registered by bh_targets_set.  Column t is read only when target
 * t is a BH_TARGET_RF, and there only for the sites that have the target (count above 0).  Host arrays [nsites][nt], copied to
 * the device together with every record's logm and first bin not formed (bh_launch_rf's expressions; the rf_no_cut tuning switch
 * is honoured at launch).  With the table bh_evaluate_sites serves the rule above.  bh_evaluate_batch and bh_rf_batch never read
 * it.  It belongs to the table of bh_sites_set_rf: whatever drops or replaces that one (bh_targets_set, every bh_sites_set*
 * entry point that registers the site table, bh_sites_set_rf itself) drops it -- register it after bh_sites_set_rf and before the
 * class tables of bh_sites_set_gauss, which it drops like every other registration.
 * BH_EINVAL: no site table; no count table (one of bh_sites_set_x .. bh_sites_set_axes); no table of bh_sites_set_rf; nsites differs
 *   from the table's; a NULL array; for a present (site, receiver-function target) pair an nsamp that is no power of two, below 4
 *   or below the site's count, an fsamp or gauss that is not finite and positive, a tshift that is not finite.
 * BH_EUNSUPPORTED: such an nsamp above BH_SITES_RF_AXIS_MAX_NSAMP. */
int bh_sites_set_rf_axis(bh_engine *e, int nsites, const int32_t *nsamp, const double *fsamp, const double *tshift, const double *gauss);

#ifdef __cplusplus
}
#endif
#endif
