/*
 * include/bh_engine_posterior_quantiles.h -- credible intervals of vs against depth of many sites: libbh_engine.so.
 *
 * An extension of include/bh_engine_posterior.h, outside the drop-in contract of include/bh_engine.h.  On the rows a
 * bh_posterior handle has loaded it selects several order statistics of every (site, depth) column of the interpolated vs in
 * one go -- what bh_posterior_columns does for the median alone -- so that the caller can form numpy.quantile(column, q,
 * method="linear") for any q without the columns ever being stored (bayhunter_amd/posterior.py: posterior_models(quantiles=)).
 * The order statistics of scalar sets (Moho depth, crustal vs, attached columns) are served by bh_posterior_scalar_quantiles
 * of include/bh_engine_posterior_datafit.h.
 *
 * The select: a radix select on the ordered key of bh_posterior_columns, 8 bits per pass -- 4 passes where the load found every
 * vs float32-exact, 8 otherwise -- and one further pass for the next key above every selected one.  A pass forms the vs of a
 * (row, depth) once and serves all R ranks from it: a key is counted for rank r where it matches r's prefix; ranks whose
 * prefixes are still equal share counters.  A workgroup is one wavefront = 64 depths of one site over a chunk of its rows; the
 * counters of the ranks that still share rank 0's prefix are private to the lane in LDS (32 KiB per workgroup, pairs of 16-bit
 * counters), the counters of the ranks that have left it are integer atomics in global memory.  Chunks meet in integer atomics
 * only: every result has the same bits on every repeat, in any row order, alone or among other sites.
 *
 * Device memory: nsites * D * R KiB of counters (BH_ENOMEM where that fails).  Errors as in bh_engine_posterior.h; BH_EINVAL and
 * BH_EUNSUPPORTED launch nothing and write nothing.
 */
#ifndef BH_ENGINE_POSTERIOR_QUANTILES_H
#define BH_ENGINE_POSTERIOR_QUANTILES_H

#include "bh_engine_posterior_datafit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Up to BH_QUANTILES_MAXRANKS order statistics of the interpolated vs of every (site, depth) column of the loaded rows.
 * dep: host [D], finite, strictly ascending, D >= 1.  R = 1 .. BH_QUANTILES_MAXRANKS.
 * rank: host [nsites][R], each < rows[site] (a site without rows takes rank 0 only).
 * lower, upper: host [nsites][D][R]: the ordered keys (bh_posterior_columns' map) of the order statistics
 *   s_(rank) and s_(min(rank + 1, n - 1)) of the column sorted ascending -- upper == lower inside a run of ties and
 *   at the last rank; both 0 for a site without rows.
 * keys32 (may be NULL): 1 where the keys are of float32 bit patterns (the load found every vs float32-exact).
 * Needs a loaded handle (bh_posterior_load), not bh_posterior_columns.  BH_EINVAL: R outside 1 .. BH_QUANTILES_MAXRANKS, D < 1
 * (or above 2^20), a dep that is not finite and strictly ascending, a rank that is not below its site's rows (or not 0 at a
 * site without rows), a handle without loaded rows, a null argument.  BH_EUNSUPPORTED: a site with 2^32 or more rows. */
int bh_posterior_column_quantiles(bh_posterior *p, int D, const double *dep, int R, const uint32_t *rank,
                                  uint64_t *lower, uint64_t *upper, int32_t *keys32);

#ifdef __cplusplus
}
#endif
#endif
