/*
 * include/bh_engine_sites_gauss.h -- sites with their OWN Gauss-law noise correlation, for libbh_engine.so.
 *
 * An extension of include/bh_engine_sites.h and include/bh_engine_sites_missing.h, outside the drop-in contract of
 * include/bh_engine.h.  A target under BH_LAW_GAUSS carries one R^-1 and one ln|R| in its descriptor (a receiver function with a
 * fixed non-zero noise correlation: the reference's usual configuration), and every site of the table shared them.  Stations fix
 * different correlations, and a station without a receiver function has none.  The entry points of this header give every site its
 * own matrix on a Gauss-law target and let a Gauss-law target be absent at some sites.
 *
 * The rule: a model of site s gets, on a Gauss-law target, the quadratic form, log-determinant, logL and misfits of a call whose
 * descriptor holds site s's own rinv / logdet_r -- the bits of the contraction of the same batch (same B, same n) run with that
 * matrix.  The sample count n and (receiver functions) the time axis stay shared.
 *
 * R^-1 depends on (correlation, n, rcond) only, so stations that fix the same value share one matrix (8 n^2 bytes: 8 MB at
 * n = 1024).  The table therefore holds correlation CLASSES, not sites: nclass matrices, nclass log-determinants and the class of
 * every site.
 */
#ifndef BH_ENGINE_SITES_GAUSS_H
#define BH_ENGINE_SITES_GAUSS_H

#include "bh_engine_sites_missing.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The most bytes the matrices of one target's table may take, nclass * n * n * 8: 1 GiB -- 128 classes at n = 1024, where an
 * array fixes a handful of distinct correlations.  (The matrices are device memory held until the table is dropped.) */
#define BH_SITES_GAUSS_MAXBYTES ((size_t)1 << 30)
/* The most classes of one target's table.  The grouping is built for a handful of classes -- the distinct correlations an array
 * fixes: one thread forms the prefixes over the classes, and every class adds a row tile to the contraction's grid. */
#define BH_SITES_GAUSS_MAXCLASSES 4096

/* The correlation classes of registered target `target` (a BH_LAW_GAUSS target of n samples) for the site table in force:
 * class_of[nsites], the class of every site, -1 where the site lacks the target; rinv[nclass][n][n], row-major matrices;
 * logdet_r[nclass].  Host arrays, copied.  bh_evaluate_sites then groups the rows of a batch by class_of[site[b]] on the device and
 * contracts every group with its own matrix; the likelihood adds the class's ln|R|.  Without a table for a target
 * bh_evaluate_sites uses the descriptor's matrix for every site, as before.  bh_evaluate_batch and bh_loglike_batch never read the
 * table.  A class no site names is allowed (it has no rows).
 * Lifetime: bh_targets_set and every bh_sites_set* entry point (bh_sites_set, _x, _x_all, _missing, _missing_gauss and _rf) drop
 *   the tables of all targets -- register them last; another call for the same target replaces its table.
 * BH_EINVAL: no site table registered; nsites differs from the table's; target out of range or not a BH_LAW_GAUSS target;
 *   nclass < 1; a class index outside [-1, nclass); a non-finite value in rinv or logdet_r; a -1 where the site has the target
 *   (count tables: a count above 0; bh_sites_set: every site has every target) or a class where the count is 0; a null pointer.
 * BH_EUNSUPPORTED: nclass above BH_SITES_GAUSS_MAXCLASSES; nclass * n * n * 8 bytes above BH_SITES_GAUSS_MAXBYTES (both checked
 *   before the arrays are read). */
int bh_sites_set_gauss(bh_engine *e, int target, int nsites, int nclass, const int32_t *class_of, const double *rinv,
                       const double *logdet_r);

/* bh_sites_set_missing that accepts a Gauss-law target which some site lacks: the same arguments, checks but that one, layout and
 * lifetime.  Such a target then NEEDS its class table (the lacking sites in class -1: their rows belong to no tile of the
 * contraction): until bh_sites_set_gauss has registered it, bh_evaluate_sites returns BH_EINVAL with a message that names
 * bh_sites_set_gauss.  bh_sites_set_missing keeps refusing that configuration. */
int bh_sites_set_missing_gauss(bh_engine *e, int nsites, const int32_t *n, const double *x, const double *yobs, const double *yerr);

#ifdef __cplusplus
}
#endif
#endif
