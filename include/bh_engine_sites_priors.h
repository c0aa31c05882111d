/*
 * include/bh_engine_sites_priors.h -- chains whose sites carry their OWN priors and sampler settings, for libbh_engine.so.
 *
 * An extension of include/bh_engine_sites_missing.h, outside the drop-in contract of include/bh_engine.h.  The chain calls so
 * far propose, validate and accept every chain of a call under ONE bh_chain_config.  The stations of a real array do not share
 * one: a basin station and a craton station have other vs / z / layer ranges, a noisy station other noise ranges, one station a
 * fixed vp/vs or the mantle rule, each its own minimum thickness, velocity-zone rules and acceptance band.  The entry points
 * of this header take a TABLE of such records and, per chain, the index of the record it runs under.
 *
 * The rule: a chain of record r walks exactly the trajectory it walks through the plain entry points with a bh_chain_config
 * that holds record r's fields -- the same moves, proposals, validity, acceptance and width adaptation, bit for bit.  (The random
 * streams depend on (seed, global chain index, iteration) only.)  What stays in bh_chain_config is what chains advanced in lock
 * step over one set of arrays must share: nt, maxlayers (the row capacity), iter_burnin, iterations, seed, chain_offset.  Its
 * station fields are not read by these entry points.
 */
#ifndef BH_ENGINE_SITES_PRIORS_H
#define BH_ENGINE_SITES_PRIORS_H

#include "bh_engine_sites_missing.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The fields of bh_chain_config that belong to a station, with their meaning there. */
typedef struct bh_chain_prior {
    int32_t layermin, layermax;    /* priors 'layers'; layermax + 1 <= cfg->maxlayers */
    double vsmin, vsmax, zmin, zmax;
    double thickmin;
    double lvz, hvz;               /* < 0 = None */
    double vpvsmin, vpvsmax;       /* equal = fixed */
    double mantle_vs, mantle_vpvs; /* mantle_vs <= 0 = None */
    double acc_lo, acc_hi;         /* [%] */
    double noise_lo[2 * BH_MAX_TARGETS], noise_hi[2 * BH_MAX_TARGETS]; /* equal = fixed */
} bh_chain_prior;

/* The four chain calls with a table: beside the arguments of their counterparts
 *   priors    device, P records;
 *   prior_of  device, int32 [C]: the record chain c runs under;
 *   absent    (the propose calls) device, uint8 [C] as in bh_chain_propose_sites, or NULL: every target present.  A noise
 *             parameter is free iff its record's noise_lo != noise_hi and its target is not absent.
 * A record is fetched once per chain at the top of each kernel.  Row capacity: cfg->maxlayers is the LARGEST capacity among the
 * records; a chain whose record has a smaller layermax meets "too many layers" in the layer-count check where its own run meets
 * it in the capacity check -- either way the proposal is invalid, with the same move and birth term, and the model it started
 * from goes to the evaluation.  The accept calls keep rows beyond n at zero up to cfg->maxlayers.
 * A chain whose prior_of is outside [0, P) reads nothing of the table: all its proposals are invalid (the evaluation sees the
 * model it holds) and the accept calls leave its state, counters included, as it was -- in band, like a site out of range.
 * BH_EINVAL: what the plain entry points refuse; null priors or prior_of; P < 1.  (With the plain entry points, these now refuse
 * a negative cfg->nt or cfg->maxlayers as well -- bh_engine.h; before, only values above the limits.) */
int bh_chain_propose_priors(void *stream, const bh_chain_config *cfg, const bh_chain_state *state, int C, int iiter,
                            const bh_chain_prior *priors, int P, const int32_t *prior_of, const uint8_t *absent);
int bh_chain_propose_window_priors(void *stream, const bh_chain_config *cfg, const bh_chain_state *state, int C, int iiter,
                                   int depth, ptrdiff_t ld, const bh_chain_prior *priors, int P, const int32_t *prior_of,
                                   const uint8_t *absent);
int bh_chain_accept_priors(void *stream, const bh_chain_config *cfg, const bh_chain_state *state, int C, int iiter,
                           const double *logL, const double *misfits, const bh_chain_prior *priors, int P,
                           const int32_t *prior_of);
int bh_chain_accept_window_priors(void *stream, const bh_chain_config *cfg, const bh_chain_state *state, int C, int iiter,
                                  int depth, ptrdiff_t ld, const double *logL, const double *misfits,
                                  const bh_chain_prior *priors, int P, const int32_t *prior_of);

#ifdef __cplusplus
}
#endif
#endif
