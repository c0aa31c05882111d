/*
 * include/bh_engine_chain_record.h -- the chains' thinned samples written on the device, for libbh_engine.so.
 *
 * An extension of include/bh_engine_sites_priors.h, outside the drop-in contract of include/bh_engine.h.  A sampler keeps the
 * chain's current model at every `thinning`-th iteration.  Taken on the host that is a synchronisation and eight copies per
 * snapshot, and a speculative window (bh_chain_accept_window) has to end at every snapshot iteration: a run that keeps every
 * iteration (thinning 1, the reference's defaults) advances one iteration per launch.  The accept kernel, however, walks the
 * realised path through the window's tree and knows the chain's state before every one of the window's iterations.  The entry
 * points of this header are the two window accept calls with a store of snapshot rows that the kernel fills on its way.
 *
 * The rule: a snapshot is due at iteration i when i mod thinning == 0, with the non-negative residue (i is negative during the
 * burn-in).  It holds the chain's state BEFORE iteration i is decided: the pre-window state if nothing was accepted at the earlier
 * levels of the window, else the proposal of the last node accepted so far with its logL and misfits.  Within one window the due
 * snapshots fill consecutive rows from row0.  The values are the float64 state rounded to nearest float32; beta is copied as
 * float64.  The decisions, the committed state, the counters and the adapted widths are those of the calls without a store, bit
 * for bit.
 */
#ifndef BH_ENGINE_CHAIN_RECORD_H
#define BH_ENGINE_CHAIN_RECORD_H

#include "bh_engine_sites_priors.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The store (device arrays, row-major; C = the call's chains, nt and maxlayers = cfg's). */
typedef struct bh_chain_record {
    float *models;    /* [rows][C][2*maxlayers]  vs_1..vs_n, z_1..z_n, NaN..  (the reference's row) */
    float *likes;     /* [rows][C] */
    float *vpvs;      /* [rows][C] */
    float *misfits;   /* [rows][C][nt+1] */
    float *noise;     /* [rows][C][2nt] */
    double *beta;     /* NULL, or [rows][C]: state->beta of the chain at that iteration */
    int64_t rows;     /* capacity */
    int64_t thinning; /* >= 1 */
    int64_t row0;     /* row of the first iteration i >= iiter of this window with i mod thinning == 0 */
} bh_chain_record;

/* bh_chain_accept_window / bh_chain_accept_window_priors with a store.  `rec` is a host structure, read during the call.
 * Both always launch the wavefront-per-chain kernel, also at depth 1 with ld == C.  With m = the number of due iterations in
 * [iiter, iiter + depth), rows row0 .. row0 + m - 1 are written for every chain; no other row is touched, and the kernel never
 * writes a row >= rows.  A chain whose prior_of is out of range keeps its state (as in bh_chain_accept_window_priors) and
 * that state is what its rows hold.
 * BH_EINVAL (nothing launched): what the calls without a store refuse (an adaptation iteration inside the window, ..); rec NULL;
 *   models, likes, vpvs, misfits or noise NULL; thinning < 1; row0 < 0; row0 + m > rows; cfg->maxlayers outside
 *   [0, BH_CHAIN_MAXLAYERS] or cfg->nt outside [0, BH_MAX_TARGETS] (these two calls always checked both bounds; every chain entry
 *   point does now -- bh_engine.h -- and that is the one return that changed anywhere when the rules were stated once). */
int bh_chain_accept_window_record(void *stream, const bh_chain_config *cfg, const bh_chain_state *state, int C, int iiter,
                                  int depth, ptrdiff_t ld, const double *logL, const double *misfits, const bh_chain_record *rec);
int bh_chain_accept_window_priors_record(void *stream, const bh_chain_config *cfg, const bh_chain_state *state, int C, int iiter,
                                         int depth, ptrdiff_t ld, const double *logL, const double *misfits,
                                         const bh_chain_prior *priors, int P, const int32_t *prior_of, const bh_chain_record *rec);

#ifdef __cplusplus
}
#endif
#endif
