/*
 * include/bh_engine_posterior_classes.h -- the loaded rows of every site split into classes by a rule over their scalar
 * columns: libbh_engine.so.
 *
 * An extension of include/bh_engine_posterior_features.h, outside the drop-in contract of include/bh_engine.h.  A
 * transdimensional posterior is often bimodal -- two Moho candidates, a low-velocity zone that is there or not -- and a summary
 * over all of a site's rows describes a model no chain sampled.  bh_posterior_classes turns a rule over the columns of the
 * scalar sets a handle has formed (BH_SCALARS_MOHO, BH_SCALARS_USER, BH_SCALARS_FEATURES; they coexist) into every row's class,
 * on the device, where the columns lie.  The caller then loads the rows again under the site index  site * K + class: a class
 * of a site is a site of its own to every call of the bh_engine_posterior*.h headers, and a row of class -1 is left out by
 * the load as every row with a site out of range is.
 *
 * The rule.  A call brings K classes and T terms.  Term t belongs to class term_class[t] (ascending, in [0, K)) and looks at
 * column term_col[t] of set term_set[t]; with v the row's float64 value there it holds where
 *   BH_CLASS_IN     v is not NaN and lo[s][t] <= v < hi[s][t], s the row's site (float64 comparisons: -0.0 equals 0.0);
 *   BH_CLASS_HAS    v is not NaN;
 *   BH_CLASS_LACKS  v is NaN.
 * A class holds for a row where all of its terms hold; a class without a term holds for every row.  The row's class is the
 * smallest k whose class holds, -1 where none does.
 *
 * Every result is a predicate on float64 values that are themselves exact functions of the rows: cls and counts are the same
 * bits alone or among other sites, in any row order (cls moves with the rows), from host or device memory, on every repeat.
 * Errors as in bh_engine_posterior.h; BH_EINVAL launches nothing and writes nothing to cls, counts or out.
 */
#ifndef BH_ENGINE_POSTERIOR_CLASSES_H
#define BH_ENGINE_POSTERIOR_CLASSES_H

#include "bh_engine_posterior_features.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BH_CLASSES_MAX 16     /* K: classes of one call */
#define BH_CLASS_MAXTERMS 64  /* T: terms of one call */

#define BH_CLASS_IN 0     /* the row has a value v in the column and lo <= v < hi */
#define BH_CLASS_HAS 1    /* the row has a value (not NaN) */
#define BH_CLASS_LACKS 2  /* the row's value is NaN */

/* Classify the rows of a load made under bh_posterior_keep_rows.  1 <= K <= BH_CLASSES_MAX, 0 <= T <= BH_CLASS_MAXTERMS;
 * term_class, term_set, term_col, term_op: host [T]; lo, hi: host [nsites][T], read for BH_CLASS_IN terms only, -inf and +inf
 * allowed, a NaN or lo > hi is BH_EINVAL, as are a set that is not formed, a column outside its set, an unknown op and a
 * term_class that does not ascend inside [0, K).
 * cls: int32 [N] in memspace (stream as in bh_posterior_load), N the rows of the loaded input, in the input's row order: the
 * row's class, -1 for a row in no class and for a row the load left out (a NaN row, an invalid row, a site out of range).
 * counts: host int64 [nsites][K + 1]: the loaded rows of site s in class k, in column K those in no class; a site's row sums
 * to rows[s] of the load. */
int bh_posterior_classes(bh_posterior *p, int K, int T, const int32_t *term_class, const int32_t *term_set,
                         const int32_t *term_col, const int32_t *term_op, const double *lo, const double *hi,
                         int memspace, void *stream, int32_t *cls, int64_t *counts);

/* The columns of a set by input row: out[i * ld + q] (float64, in memspace, ld >= the set's columns) is column q of input row
 * i, NaN in every column for a row the load left out; elements at q >= the set's columns are not touched.  What a rule the
 * term table cannot express is written from, and what lets one set's column be plotted against another's. */
int bh_posterior_scalar_export(bh_posterior *p, int set, int memspace, void *stream, int64_t ld, double *out);

#ifdef __cplusplus
}
#endif
#endif
