// bayhunter_amd/csrc/chain_step.hip -- the launch plan of the chain step (chain_step.h): every rule of the twelve bh_chain_* entry
// points, once.  Host code only: no kernel, no HIP call, nothing static -- the plan is a function of the ask alone.
#include "chain_step.h"

namespace {

// what an entry point is, by its place in ChainEntry
struct EntryKind {
    bool accept;  // an accept call (logL and misfits required), else a propose call
    bool window;  // takes depth and ld (else depth 1, ld = C)
    bool absent;  // requires the absent mask
    bool table;   // requires priors, prior_of and P >= 1
    bool record;  // requires a store; always the wavefront-per-chain kernel
};
const EntryKind KIND[CHAIN_ENTRIES] = {
    {false, false, false, false, false}, // CHAIN_PROPOSE
    {true, false, false, false, false},  // CHAIN_ACCEPT
    {false, true, false, false, false},  // CHAIN_PROPOSE_WINDOW
    {true, true, false, false, false},   // CHAIN_ACCEPT_WINDOW
    {false, false, true, false, false},  // CHAIN_PROPOSE_SITES
    {false, true, true, false, false},   // CHAIN_PROPOSE_WINDOW_SITES
    {false, false, false, true, false},  // CHAIN_PROPOSE_PRIORS
    {false, true, false, true, false},   // CHAIN_PROPOSE_WINDOW_PRIORS
    {true, false, false, true, false},   // CHAIN_ACCEPT_PRIORS
    {true, true, false, true, false},    // CHAIN_ACCEPT_WINDOW_PRIORS
    {true, true, false, false, true},    // CHAIN_ACCEPT_WINDOW_RECORD
    {true, true, false, true, true},     // CHAIN_ACCEPT_WINDOW_PRIORS_RECORD
};

ChainStepPlan refuse(int code)
{
    ChainStepPlan p{};
    p.code = code;
    return p;
}

} // namespace

ChainStepPlan bh_plan_chain_step(const ChainStepAsk &q)
{
    if (q.entry < 0 || q.entry >= CHAIN_ENTRIES) return refuse(BH_EINVAL);
    const EntryKind &E = KIND[q.entry];
    const int C = q.C, depth = E.window ? q.depth : 1;
    const int64_t ld = E.window ? q.ld : (int64_t)C;

    // ---- the arguments ---------------------------------------------------------------------------------------------------------
    if (!q.cfg || !q.state || C < 0) return refuse(BH_EINVAL);
    if (q.nt < 0 || q.nt > BH_MAX_TARGETS || q.maxlayers < 0 || q.maxlayers > BH_CHAIN_MAXLAYERS) return refuse(BH_EINVAL);
    if (depth < 1 || depth > BH_CHAIN_MAXDEPTH) return refuse(BH_EINVAL);
    const int N = (1 << depth) - 1; // the nodes of a chain's tree
    if (ld < (int64_t)C * N) return refuse(BH_EINVAL);
    if (E.accept && (!q.logL || !q.misfits)) return refuse(BH_EINVAL);
    if (E.absent && !q.absent) return refuse(BH_EINVAL);
    if (E.table && (!q.priors || !q.prior_of || q.P < 1)) return refuse(BH_EINVAL);
    for (int k = 0; k + 1 < depth; ++k)
        if (((int64_t)q.iiter + k) % 1000 == 0) return refuse(BH_EINVAL); // an adaptation iteration must be the last of its window

    ChainStepPlan p{};
    if (E.record) {
        if (!q.rec || !q.rec_models || !q.rec_likes || !q.rec_vpvs || !q.rec_misfits || !q.rec_noise) return refuse(BH_EINVAL);
        if (q.thinning < 1 || q.row0 < 0) return refuse(BH_EINVAL);
        // the first due level: iiter + first = 0 mod thinning (non-negative residue); m due levels in the window
        const int64_t res = (((int64_t)q.iiter % q.thinning) + q.thinning) % q.thinning;
        const int64_t first = res == 0 ? 0 : q.thinning - res;
        const int64_t m = first >= depth ? 0 : 1 + ((int64_t)depth - 1 - first) / q.thinning;
        if (q.row0 > q.rows - m) return refuse(BH_EINVAL);
        // (a step beyond the deepest window means "no further one": thinning itself need not fit an int)
        p.due = (int)(first < depth ? first : depth);
        p.due_step = (int)(q.thinning <= BH_CHAIN_MAXDEPTH ? q.thinning : BH_CHAIN_MAXDEPTH + 1);
        p.m = (int)m;
    }
    if (C == 0) return p; // (after every check: BH_OK, nothing to launch)

    // ---- the kernel and its geometry -------------------------------------------------------------------------------------------
    p.block = 64;
    if (E.accept) {
        const bool wave = E.record || depth > 1; // a wavefront per chain; a lane per chain for the plain accept step
        p.kernel = wave ? CHAIN_KERNEL_ACCEPT_WAVE : CHAIN_KERNEL_ACCEPT_LANE;
        p.grid = wave ? (unsigned)C : ((unsigned)C + 63u) / 64u;
    } else if (depth == 1 && ld == C) {
        p.kernel = CHAIN_KERNEL_PROPOSE_LANE;
        p.grid = ((unsigned)C + 63u) / 64u;
    } else {
        const int per_wg = 64 >> (depth - 1); // chains of a single-wavefront workgroup
        // the tree (odd record stride), then with a table of priors the noise bounds of the workgroup's chains
        p.lds = ((size_t)per_wg * N * (node_rec_doubles(q.nt, q.maxlayers) | 1) + (E.table ? (size_t)per_wg * 4 * BH_MAX_TARGETS : 0)) *
                sizeof(double);
        if (p.lds > 160 * 1024) return refuse(BH_EUNSUPPORTED);
        p.big_lds = p.lds > 64 * 1024;
        p.kernel = CHAIN_KERNEL_PROPOSE_WINDOW;
        p.grid = ((unsigned)C + per_wg - 1) / per_wg;
    }
    return p;
}
