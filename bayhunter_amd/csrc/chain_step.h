// bayhunter_amd/csrc/chain_step.h -- what a chain-step entry point asks and what it is told: the launch plan of the twelve bh_chain_*
// calls (include/bh_engine.h, bh_engine_sites_missing.h, bh_engine_sites_priors.h, bh_engine_chain_record.h).
//
// Host only, no HIP type: an entry point fills a ChainStepAsk from its arguments (whether a pointer is null, never the pointer),
// bh_plan_chain_step (chain_step.hip; pure: no HIP call, no allocation, nothing static) states every rule once -- the argument
// checks, the kernel, its geometry and LDS, the record kernels' due levels -- and the entry point launches what the plan names,
// with the kernels of its own translation unit (chain_kernel.hip, five builds).  tests/test_chain_step_plan.py holds the planner to
// the recorded refusals of the entry points before it and to a restatement of the geometry, without a GPU.
#ifndef BH_CHAIN_STEP_H
#define BH_CHAIN_STEP_H

#include "../../include/bh_engine_chain_record.h"

// LDS record of one tree node of the window propose kernel (doubles): [0] n  [1] valid  [2] vp/vs  [3 .. 3+2nt) noise  then
// vs[ML+1], z[ML+1], h[ML+1].  (constexpr: callable from the kernel and from the planner alike.)
constexpr int node_rec_doubles(int nt, int ML) { return 3 + 2 * nt + 3 * (ML + 1); }

// the twelve entry points, in the order of their headers
enum ChainEntry {
    CHAIN_PROPOSE = 0,                 // bh_engine.h
    CHAIN_ACCEPT,
    CHAIN_PROPOSE_WINDOW,
    CHAIN_ACCEPT_WINDOW,
    CHAIN_PROPOSE_SITES,               // bh_engine_sites_missing.h: absent[C] required
    CHAIN_PROPOSE_WINDOW_SITES,
    CHAIN_PROPOSE_PRIORS,              // bh_engine_sites_priors.h: a table of priors required, absent optional
    CHAIN_PROPOSE_WINDOW_PRIORS,
    CHAIN_ACCEPT_PRIORS,
    CHAIN_ACCEPT_WINDOW_PRIORS,
    CHAIN_ACCEPT_WINDOW_RECORD,        // bh_engine_chain_record.h: a store required
    CHAIN_ACCEPT_WINDOW_PRIORS_RECORD,
    CHAIN_ENTRIES
};

enum ChainKernel {
    CHAIN_KERNEL_NONE = 0,        // nothing to launch: the plan's code is the call's result
    CHAIN_KERNEL_PROPOSE_LANE,    // chain_propose_kernel: a lane per chain, one proposal
    CHAIN_KERNEL_PROPOSE_WINDOW,  // chain_propose_window_kernel: 2^(depth-1) lanes per chain, the tree in dynamic LDS
    CHAIN_KERNEL_ACCEPT_LANE,     // chain_accept_kernel: a lane per chain
    CHAIN_KERNEL_ACCEPT_WAVE      // chain_accept_window_kernel: a wavefront per chain
};

struct ChainStepAsk {
    int entry;              // ChainEntry
    bool cfg, state;        // non-null
    int nt, maxlayers;      // cfg's (0 with a null cfg)
    int C, iiter, depth;    // (the entries without a depth: depth 1, ld = C, whatever these say)
    int64_t ld;
    bool logL, misfits, absent, priors, prior_of; // non-null
    int P;
    bool rec, rec_models, rec_likes, rec_vpvs, rec_misfits, rec_noise; // the store and its float arrays, non-null
    int64_t rows, thinning, row0;                                      // the store's (0 with a null store)
};

struct ChainStepPlan {
    int code;               // BH_OK, or why nothing is launched (BH_EINVAL, BH_EUNSUPPORTED)
    int kernel;             // ChainKernel; CHAIN_KERNEL_NONE with a refusal and with C == 0
    unsigned grid, block;
    size_t lds;             // dynamic LDS [bytes]
    bool big_lds;           // lds exceeds the 64 KiB every kernel may have: the kernel needs the 160 KiB allowance first
    int due, due_step;      // record kernels: the first due level of the window (depth: none) and the levels between due ones
    int m;                  // record entries: the due levels in the window (rows row0 .. row0 + m - 1 are written)
};

ChainStepPlan bh_plan_chain_step(const ChainStepAsk &q);

// The part of the ask that every entry point fills the same way.
inline ChainStepAsk chain_step_ask(ChainEntry entry, const bh_chain_config *cfg, const bh_chain_state *state, int C, int iiter, int depth,
                                   ptrdiff_t ld)
{
    ChainStepAsk q{};
    q.entry = entry;
    q.cfg = cfg != nullptr;
    q.state = state != nullptr;
    q.nt = cfg ? cfg->nt : 0;
    q.maxlayers = cfg ? cfg->maxlayers : 0;
    q.C = C; q.iiter = iiter; q.depth = depth; q.ld = (int64_t)ld;
    return q;
}
// ... and of a table of priors (all null for the entries without one) and of a store (null for the entries without one)
inline void chain_step_ask_table(ChainStepAsk &q, const uint8_t *absent, const bh_chain_prior *priors, int P, const int32_t *prior_of)
{
    q.absent = absent != nullptr;
    q.priors = priors != nullptr;
    q.prior_of = prior_of != nullptr;
    q.P = P;
}
inline void chain_step_ask_record(ChainStepAsk &q, const bh_chain_record *rec)
{
    q.rec = rec != nullptr;
    if (!rec) return;
    q.rec_models = rec->models != nullptr; q.rec_likes = rec->likes != nullptr; q.rec_vpvs = rec->vpvs != nullptr;
    q.rec_misfits = rec->misfits != nullptr; q.rec_noise = rec->noise != nullptr;
    q.rows = rec->rows; q.thinning = rec->thinning; q.row0 = rec->row0;
}
#endif
