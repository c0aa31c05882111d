// bayhunter_amd/csrc/engine_swd.hip -- the dispersion part of the engine's host side (bh_engine_impl.h): the plan of a call's dispersion
// jobs (plan_swd: kernel, lanes per model, trials per round, processing order), its work space and its launches -- ordering, main
// launch, re-run of guarded models, second roots -- and bh_swd_batch.  The kernels are those of swd_kernel.hip, swd_group_*.hip and
// swd_lean.hip behind the launchers of bh_device.h.
#include "bh_engine_impl.h"

using namespace bheng;

namespace {

// prologue: null, or the fills of the call's ordering launch (SwdPlan::prologue), which then zeroes the counters
int swd_counter(bh_engine *e, hipStream_t st, SwdFills *prologue, unsigned long long **out)
{
    *out = nullptr;
    if (!e->counting) return BH_OK;
    int rc = ensure(e, e->counter, BH_DEBUG_WORDS * sizeof(unsigned long long));
    if (rc) return rc;
    if (!e->neval_pending) {
        if (prologue) {
            prologue->counter = (unsigned long long *)e->counter.p;
            prologue->ncounter = BH_COUNTER_WORDS;
        } else {
            HIPCHK(e, hipMemsetAsync(e->counter.p, 0, BH_COUNTER_WORDS * sizeof(unsigned long long), st));
        }
        e->neval_pending = true;
    }
    *out = (unsigned long long *)e->counter.p;
    return BH_OK;
}

// The guard of the short refinement (SearchT, swd_common.h): work space = three blocks of BH_MAX_TARGETS counts (GUARD_HEAD = 24 words, below) followed by one
// list of B model indices per target.  prologue: null, or the fills of the call's ordering launch (SwdPlan::prologue), which then
// zeroes the head's words.
int guard_space(bh_engine *e, hipStream_t st, int B, SwdFills *prologue, int32_t **counts, int32_t **lists)
{
    const size_t need = ((size_t)GUARD_HEAD + (size_t)BH_MAX_TARGETS * (size_t)(B + 4)) * sizeof(int32_t);
    if (need > e->guard.cap) { // (a new buffer: carry the cumulative counts over on the host side)
        if (e->guard.p) {
            int32_t cum[BH_MAX_TARGETS];
            HIPCHK(e, hipStreamSynchronize(st));
            HIPCHK(e, hipMemcpy(cum, (int32_t *)e->guard.p + 2 * BH_MAX_TARGETS, sizeof(cum), hipMemcpyDeviceToHost));
            for (int t = 0; t < BH_MAX_TARGETS; ++t) e->guard_total[t] += (uint64_t)(uint32_t)cum[t]; // (the device word wraps as unsigned)
        }
        e->guard_fresh = true;
    }
    int rc = ensure(e, e->guard, need);
    if (rc) return rc;
    *counts = (int32_t *)e->guard.p;
    *lists = (int32_t *)e->guard.p + GUARD_HEAD;
    // words [0, 8): this call's lists' lengths (re-run launch); [8, 16): this call's models restarted in place (group kernel,
    // one model per wavefront); [16, 24): cumulative since the buffer was made
    const int words = e->guard_fresh ? GUARD_HEAD : 2 * BH_MAX_TARGETS;
    if (prologue) {
        prologue->guard = (int32_t *)e->guard.p;
        prologue->nguard = words;
    } else {
        HIPCHK(e, hipMemsetAsync(e->guard.p, 0, (size_t)words * sizeof(int32_t), st));
    }
    e->guard_fresh = false;
    return BH_OK;
}

// which jobs take the short refinement: fundamental-mode phase velocities; with BH_SEARCH_FAST_RAYLEIGH only the Rayleigh ones
bool takes_fast(int search, const SwdJob &J)
{
    return J.igr == BH_VEL_PHASE && J.mode <= 1 && (search == BH_SEARCH_FAST || (search == BH_SEARCH_FAST_RAYLEIGH && J.iwave == BH_WAVE_RAYLEIGH));
}

// processing order of the models: the caller's; deepest first (models of more than Lcut layers a class of their own:
// SwdMultiArgs::split); by predicted search length (trial-per-lane kernel, PairOrderTarget); paired over the SIMDs (SwdPairWork)
enum SwdOrder { ORDER_NONE = BH_ORDER_NONE, ORDER_DEPTH = BH_ORDER_DEPTH, ORDER_LENGTH = BH_ORDER_LENGTH, ORDER_PAIR = BH_ORDER_PAIR }; // (bh_engine_last_swd_order)

// The plan of one dispersion call, from the engine's settings, the experiment switches (bh_tuning.h) and the call's shape:
// no HIP call, no allocation.  typ_given: the batch's typical layer count (0 = unknown).
//   Periods per site (a job with SwdSiteJob::tab; then every job of the call has it): the site-period builds of the trial-per-lane
// and group kernels keep a row of kmax periods for EACH model of a wavefront, so LDS is sized for "periods per model" (p.sitex).
// Where the trial-per-lane kernel then asks for more than a workgroup's LDS -- few trials per round are many models per
// wavefront: 4 trials = 16 models x 60 periods x 8 B beside 16 models of 16 layers are 86 KB -- the call falls back to the group
// kernel, as it does for deep arrays.  The one-lane-per-evaluation kernel (swd_kernel) has no site-period build of a main launch: such
// calls take at least two lanes per model (the group kernel), as deep arrays already do.  (Its launch of second roots has one:
// launch_second_roots, for the tables of bh_sites_set_x_all.)
SwdPlan plan_swd(const bh_engine *e, int B, int Lmax, int typ_given, int njobs, const SwdJob *jobs)
{
    const BhTuning &tun = bh_tuning();
    SwdPlan p{};
    p.maxmode = 1;
    for (int j = 0; j < njobs; ++j) p.sitex = p.sitex || jobs[j].sx.tab != nullptr;
    int iw[BH_MAX_TARGETS], nfast = 0;
    for (int j = 0; j < njobs; ++j) {
        const SwdJob &J = jobs[j];
        if (J.K == 0) continue;
        // Group velocities of the fundamental mode: two launches.  The root at t/(1+h) of period k + 1 starts from the root at
        // t/(1+h) of period k (surfdisp96.f:262-266); the root at t/(1-h) starts from the root at t/(1+h) of ITS OWN period
        // (:282-287) and nothing starts from it.  One search after the other is a chain of 2 K dependent roots; here the target
        // first runs as the chain of its K first roots (beside the call's other targets, in whatever kernel the call takes,
        // every root stored unrounded in the output row), then a launch of B x K independent searches (one lane each, or up to
        // 16 trial lanes while that still fits the chip at once: launch_second_roots) finds the second roots and puts the group
        // velocities in their place.  The same searches on the same values: the same bits (tests/test_gpu_swd.py's golden rows
        // and oracle comparisons run through here).  Measured, one launch -> two (ms per call): one model 2.26 -> 1.43; two
        // targets x 256 / 1024 / 4096 / 8192 / 16 384 / 65 536 models: 2.64 -> 1.90, 2.91 -> 2.10, 5.51 -> 4.64, 11.2 -> 8.09,
        // 17.2 -> 12.5, 31.5 -> 29.9 (the second roots are a third of the evaluations but run as full wavefronts of independent
        // searches, one lane each; in one launch they sit in the chain's wavefronts, whose lanes wait for each other's searches).
        // bh_tuning.h swd_gsplit: the largest call in (model, period) pairs that is split (0: none).
        p.first_roots[j] = J.igr == BH_VEL_GROUP && J.mode <= 1 && tun.swd_gsplit > 0 && (long)B * J.K <= (long)tun.swd_gsplit;
        p.nsplit += p.first_roots[j] ? 1 : 0;
        const int t = p.ntargets++;
        p.job[t] = j;
        iw[t] = J.iwave;
        p.fast[t] = takes_fast(e->swd_search, J);
        nfast += p.fast[t] ? 1 : 0;
        p.kmax = J.K > p.kmax ? J.K : p.kmax;
        p.maxmode = J.mode > p.maxmode ? J.mode : p.maxmode;
        p.any_sphere = p.any_sphere || J.flsph == 1;
    }
    const int nlive = p.ntargets;
    if (nlive == 0) return p;
    // Typical depth of the batch (0 = unknown: the array capacity is planned for).  Ignored where every (model, target) gets a
    // wavefront of its own anyway (at most 2048 of them: the chip's two per SIMD) -- the regime of the chains' speculative
    // windows.  There a depth class of its own for the shallow bulk buys nothing (the models per wavefront cannot grow), the
    // narrower lane groups cost a second pass over the layers and seven instead of four trials per round more transitions:
    // measured on windows of 1016 models of 3-9 layers in arrays of 21 (c4): 1.50 ms without the hint, 1.70-1.83 ms with it.
    p.typ_layers = ((long)nlive * B <= 2048 && tun.swd_hint_always == 0) ? 0 : typ_given;
    int look[BH_MAX_TARGETS];
    {
        // lanes per model follow the TYPICAL depth of the batch (deeper models take further passes over
        // their layers): known for host batches, a caller's hint for device-resident ones, else Lmax
        int Lplan = p.typ_layers > 0 ? p.typ_layers : Lmax;
        if (Lplan > Lmax) Lplan = Lmax;
        bh_swd_plan(B, Lplan, nlive, iw, e->force_group, &p.G, look);
        if (e->force_look > 0)
            for (int t = 0; t < nlive; ++t) look[t] = e->force_look; // (one lane per model: rounded down to a power of two)
    }
    const size_t lds_cap = 64 * 1024;
    if (p.G <= 1 && (p.sitex || bh_swd_lds_bytes(Lmax, p.kmax, p.maxmode) > lds_cap)) p.G = 2; // deep models / many periods / periods per site
    // The trial-per-lane kernel (swd_lean.hip): every target of the call takes the short refinement with the fast arithmetic, in
    // calls of up to 2^20 (model, target) pairs (with four trials per round it stays ahead of one lane per evaluation -- swd_kernel's
    // FA builds -- as far as measured: c2 at B = 65 536 7.99 against 8.44 ms).
    {
        bool all = e->swd_arith == BH_ARITH_FAST && e->swd_search == BH_SEARCH_FAST && e->force_group == 0 && e->force_look == 0 &&
                   tun.swd_look_r == 0 && tun.swd_look_l == 0 && tun.swd_no_lean == 0 && p.maxmode <= 1 && p.kmax <= BH_MAX_PERIODS &&
                   Lmax <= 32 && (long)B * nlive <= (tun.swd_lean_pairs > 0 ? (long)tun.swd_lean_pairs : (1L << 20));
        for (int t = 0; t < nlive; ++t) all = all && jobs[p.job[t]].igr == BH_VEL_PHASE;
        if (all) p.lean_trials = e->swd_trials > 0 ? e->swd_trials : bh_swd_lean_trials(B, nlive);
        if (p.lean_trials >= 4 && bh_swd_lean_lds_bytes(p.lean_trials, Lmax, p.kmax, p.sitex) > lds_cap) p.lean_trials = 0; // (a workgroup's LDS)
    }
    const bool lean = p.lean_trials >= 4;
    if (lean && p.G <= 1) p.G = bh_swd_pick_group(B, nlive, Lmax); // (the launch is set up where the group kernel's is)
    p.kernel = p.G <= 1 ? BH_KERNEL_LANE : (lean ? BH_KERNEL_LEAN : BH_KERNEL_GROUP);
    // processing order: deepest models first, wavefronts of (nearly) one depth
    const bool ordered = B > 1 && tun.no_order == 0 && !e->as_given;
    const bool shallow_bulk = p.typ_layers > 0 && p.typ_layers + 2 < Lmax;
    // One depth class, lanes per model > 1: the models by predicted search length, paired over the SIMDs (SwdPairWork; at
    // the lanes the group kernel's plan launches, order_models); mixed depths are ordered by depth.
    // Measured (bench.py c2, B = 2048 ... 4096, same session with / without): -3 % at 4096 and -4 % at 3800, where the
    // launch nearly fills two wavefronts per SIMD and the Rayleigh wavefronts (look-ahead 2) outnumber the Love ones
    // (trials inside the lane groups) 7 : 3; neutral at 3500; +2.5 % at 2048 / 3072, where the planner gives both targets
    // the same look-ahead and every SIMD holds one Rayleigh and one Love wavefront (why the one-to-one mix loses is not
    // understood).  Hence: two targets, >= 7/8 of two wavefronts per SIMD, unequal wavefront counts.
    if (ordered && !lean && tun.swd_no_pair == 0 && p.G > 1 && nlive == 2 && bh_pair_order_fits(B) && !shallow_bulk) {
        long plan_waves = 0, wmin = 0, wmax = 0;
        for (int t = 0; t < nlive; ++t) {
            const int mpw = BH_WAVE / (p.G * bh_trials_fit(p.G, look[t]));
            const long w = (B + mpw - 1) / mpw;
            plan_waves += w;
            wmin = (t == 0 || w < wmin) ? w : wmin;
            wmax = w > wmax ? w : wmax;
        }
        const int pair_min = tun.swd_pair_minwaves;
        if (plan_waves >= (pair_min >= 0 ? pair_min : 7 * (long)e->pairwork.ncu) && (pair_min >= 0 || 2 * wmax >= 3 * wmin))
            p.order = ORDER_PAIR;
    }
    p.Lcut = Lmax;
    if (ordered && p.order != ORDER_PAIR) {
        if (lean && bh_pair_order_fits(B) && tun.swd_lean_no_sort == 0) {
            // The trial-per-lane kernel: the models in the order of their PREDICTED search length, longest first (mixed depths:
            // deepest first) -- wavefronts of like models idle fewer rounds on finished ones, and the long wavefronts are
            // dispatched first with the short ones filling the launch's tail (c2: 0.79 -> 0.72 ms).  Scheduling only.
            // Sorted inside eight blocks of the batch, block x for the wavefronts of XCD x, where the shapes divide: each XCD's L2
            // then fetches an eighth of the model arrays instead of all of them (HBM reads of the launch 10.7 -> 1.9 MB at c2).
            p.order = ORDER_LENGTH;
            p.len_mpw = 1;
            const int mpw = BH_WAVE / p.lean_trials, per_wg = (nlive == 2) ? 2 : 4;
            if (tun.swd_lean_xcd != 0 && tun.swd_lean_r < 4 && tun.swd_lean_l < 4 && B % mpw == 0 && B % 8 == 0 && (B / mpw) % (8 * per_wg) == 0) {
                p.len_mpw = mpw;
                p.len_xcd = per_wg;
            }
        } else {
            // LDS rows for the bulk of the batch: its typical depth plus a margin; deeper models get their own launch
            p.order = ORDER_DEPTH;
            if (shallow_bulk) p.Lcut = p.typ_layers + 2;
        }
    }
    p.prologue = p.order == ORDER_LENGTH || p.order == ORDER_PAIR;
    // trials per round and sequence of every target
    p.any_fast = nfast > 0;
    p.farith = e->swd_arith == BH_ARITH_FAST;
    p.adapt_ok = e->force_group == 0 && e->force_look == 0 && tun.swd_look_r == 0 && tun.swd_look_l == 0;
    for (int t = 0; t < nlive; ++t) {
        // Where some phase-velocity targets take the short refinement and others keep the reference's sequence
        // (BH_SEARCH_FAST_RAYLEIGH with Love targets in the call) the ONE launch of the group kernel takes the build with both
        // sequences and the targets say which is theirs (two launches side by side were measured: the Rayleigh / Love pairs on
        // the SIMDs are lost, c4 1.37 -> 1.58 ms per window).
        p.refseq[t] = nfast > 0 && jobs[p.job[t]].igr == BH_VEL_PHASE && !p.fast[t];
        if (p.kernel == BH_KERNEL_LANE) { // (a launch per target: one lane per trial)
            p.look[t] = look[t] > 1 ? look[t] : 1;
            continue;
        }
        // Love: two trials inside each lane group pay while the group count is small (measured: wavefront
        // 7 % shorter at look = 1, neutral at 2, slower beyond)
        p.inlook[t] = (iw[t] != BH_WAVE_LOVE) ? 1 : (tun.swd_love_inlook > 0 ? tun.swd_love_inlook : (look[t] <= 2 ? 2 : 1));
        int L = look[t];
        if (tun.swd_look_r > 0 && iw[t] == BH_WAVE_RAYLEIGH) L = tun.swd_look_r;
        if (tun.swd_look_l > 0 && iw[t] == BH_WAVE_LOVE) L = tun.swd_look_l;
        p.look_group[t] = L;
        if (lean) {
            L = p.lean_trials;
            if (iw[t] == BH_WAVE_RAYLEIGH && tun.swd_lean_r >= 4) L = tun.swd_lean_r;
            if (iw[t] == BH_WAVE_LOVE && tun.swd_lean_l >= 4) L = tun.swd_lean_l;
        }
        p.look[t] = L;
    }
    return p;
}

// The group kernel's launch of a call planned by plan_swd (BH_KERNEL_GROUP)
SwdGroupPlan plan_group(const bh_engine *e, const SwdPlan &p, int B, int Lmax, const SwdJob *jobs)
{
    SwdGroupAsk q{};
    q.B = B; q.Lmax = Lmax; q.Lcut = p.Lcut; q.ntargets = p.ntargets; q.G0 = p.G;
    for (int t = 0; t < p.ntargets; ++t) {
        const SwdJob &J = jobs[p.job[t]];
        q.t[t] = SwdGroupAsk::Target{J.K, p.look[t], J.iwave, J.mode, J.igr != BH_VEL_PHASE, p.refseq[t]};
    }
    q.fast = p.any_fast; q.farith = p.farith;
    q.restart = true; // (takes effect in launches of one model per wavefront)
    q.adapt_ok = p.adapt_ok; q.counters = e->counting; q.scan = e->swd_scan; q.sitex = p.sitex;
    return bh_plan_swd_group(q, bh_tuning());
}

// One dispersion call as it is launched: its plan, the model arrays and work space the launches read.
struct SwdCall {
    bh_engine *e; hipStream_t st;
    const ModelBatch &m;
    const SwdJob *jobs; const SwdPlan &p;
    const double *sph = nullptr;         // flsph = 1: earth-flattened h, vp, vs, Love rho, Rayleigh rho, [Lmax][B] each
    double *first[BH_MAX_TARGETS] = {};  // per job of the chain of first roots: where the kernel keeps them (SwdKernelArgs::first)
    SwdGroupPlan g{};                    // the group kernel's launch (BH_KERNEL_GROUP)
    const int32_t *perm = nullptr, *split = nullptr;
    const int32_t *pair_perm[2] = {};    // ORDER_PAIR: the order of target 0 / 1 (SwdTarget::perm)
    unsigned long long *counter = nullptr;
    int32_t *gcounts = nullptr, *glists = nullptr; // the guard of the short refinement (guard_space)
    SwdFills fills{};                    // p.prologue: what the ordering launch zeroes
    int order_wgs = 0;                   // workgroups of the ordering launch (0: none)
    SwdSiteXArgs sx{};                   // p.sitex: the period table with the launch's targets (launch_swd_multi)
    int prio_low = 0;                    // the main launch's SwdMultiArgs::prio_low (EvalPlan::prio_low)
    SwdLaunchInfo info{};                // of the group or trial-per-lane kernel's main launch (workgroups == 0: none)
};

// The kernel arguments of job j as a target: its model arrays (the batch's, or the flattened copies with the density of its wave
// type), periods and outputs.  igr = 2 tells the kernels that a job is the chain of first roots (SwdKernelArgs::first).
SwdTarget swd_target(const SwdCall &c, int j)
{
    const SwdJob &J = c.jobs[j];
    SwdTarget t{};
    t.iwave = J.iwave; t.igr = c.p.first_roots[j] ? 2 : J.igr; t.K = J.K; t.ldv = J.ldv; t.mode = J.mode;
    t.h = c.m.h; t.vp = c.m.vp; t.vs = c.m.vs; t.rho = c.m.rho; t.sl = c.m.sl; t.sb = c.m.sb;
    if (J.flsph == 1) {
        const size_t ne = (size_t)c.m.Lmax * c.m.B;
        t.h = c.sph; t.vp = c.sph + ne; t.vs = c.sph + 2 * ne; t.rho = c.sph + (J.iwave == BH_WAVE_LOVE ? 3 : 4) * ne;
        t.sl = c.m.B; t.sb = 1;
    }
    t.periods = J.periods_dev; t.vel = J.vel; t.err = J.err;
    t.first = c.first[j];
    return t;
}

// the one-lane-per-model kernel's arguments of a target
SwdKernelArgs lane_args(const SwdCall &c, const SwdTarget &t)
{
    SwdKernelArgs a{};
    a.B = c.m.B; a.Lmax = c.m.Lmax; a.K = t.K; a.igr = t.igr; a.mode = t.mode; a.perm = c.perm;
    a.nlay = c.m.nlay; a.h = t.h; a.vp = t.vp; a.vs = t.vs; a.rho = t.rho; a.sl = t.sl; a.sb = t.sb;
    a.periods = t.periods; a.vel = t.vel; a.ldv = t.ldv; a.err = t.err; a.first = t.first;
    a.neval = c.counter; a.counted = c.e->swd_scan;
    return a;
}

// progress board of the group kernel (scheduling aid; zeroed once, entries carry a launch stamp)
int swd_board(bh_engine *e, hipStream_t st, unsigned **board)
{
    if (!e->board.p) {
        int rc = ensure(e, e->board, (size_t)BH_BOARD_WORDS * sizeof(unsigned));
        if (rc) return rc;
        HIPCHK(e, hipMemsetAsync(e->board.p, 0, (size_t)BH_BOARD_WORDS * sizeof(unsigned), st));
    }
    *board = (unsigned *)e->board.p;
    return BH_OK;
}

// the next launch stamp of the group kernel (16 bits, never 0)
unsigned swd_stamp(bh_engine *e)
{
    const unsigned s = (++e->swd_stamp) & 0xffffu;
    return s != 0 ? s : (++e->swd_stamp) & 0xffffu;
}

// One launch of the current call for bh_engine_last_swd_launches (host side: the plans' and launchers' own choices)
void note_launch(bh_engine *e, int family, int role, const int key[6], bool two, bool inter, bool pair, bool restart, unsigned grid_x, int fair)
{
    if (e->n_swd_launches >= (int)(sizeof(e->swd_launches) / sizeof(e->swd_launches[0]))) return;
    bh_swd_launch &r = e->swd_launches[e->n_swd_launches++];
    r.family = family; r.role = role;
    for (int k = 0; k < 6; ++k) r.key[k] = key[k];
    r.two_classes = two; r.interleaved = inter; r.pair_order = pair; r.restart = restart; r.grid_x = (int)grid_x; r.fair = fair;
}
void note_lane(bh_engine *e, int role, const SwdLaneBuild &b) { note_launch(e, BH_KERNEL_LANE, role, b.key, false, false, false, false, b.grid_x, b.fair); }
void note_group(bh_engine *e, int role, const SwdGroupPlan &g, bool pair)
{
    const SwdGroupBuild &b = g.build;
    const int key[6] = {b.fastm, b.simple, b.prof, b.adapt, b.cntb, b.fa};
    note_launch(e, BH_KERNEL_GROUP, role, key, g.grid.z == 2, g.wg_n1 > 0, pair, g.restart, g.grid.x, 0);
}

// The group kernel's decisions (bh_plan_swd_group) in its arguments a
void set_group_args(SwdMultiArgs &a, const SwdGroupPlan &g)
{
    for (int k = 0; k < 2; ++k) {
        a.rows[k] = g.rows[k];
        a.lanes[k] = g.lanes[k];
    }
    a.wg_n0 = g.wg_n0;
    a.wg_n1 = g.wg_n1;
    a.fast = g.build.fastm;
    a.counted = g.build.cntb ? 1 : 0;
    a.farith = g.build.fa ? 1 : 0;
    a.restart = g.restart ? 1 : 0;
}

// Load ranks of the wavefronts of a launch for the SIMD-pairing order (SwdPairWork).  Placement rule of the workgroup
// dispatcher, read off the wavefront trace (tools/gpu_trace.py, MAP=...; identical from run to run): workgroup g of a
// one-dimensional grid runs on CU g mod ncu in pass g / ncu, and its two wavefronts sit on SIMD (pass + j) mod 4 -- so SIMD
// s of a CU holds wavefront 0 of its pass-s workgroup and wavefront 1 of its pass-(s-1) workgroup, and the SIMDs whose
// partner workgroup does not exist (the last pass is not full) hold one wavefront only.
// Every wavefront gets a wanted load quantile q (0 = longest models): 0 for a wavefront alone on its SIMD, u and 1 - u for
// the two of a pair (u spread over (0, 1/2) across the pairs); per target the wavefronts are ranked by q.
bool build_slot_ranks(int n0, int n1, int ncu, std::vector<int32_t> rank[2])
{
    const int NW = n0 + n1, nwg = (NW + 1) / 2;
    if (ncu <= 0 || nwg > 4 * ncu) return false; // more than one round of workgroups: placement not fixed by the index
    auto target_of = [&](int W, int &ty, int &wid) {
        if (n1 > 0) {
            const long long N = NW;
            const int l0 = (int)(((long long)W * n1) / N), l1 = (int)((((long long)W + 1) * n1) / N);
            ty = (l1 > l0) ? 1 : 0;
            wid = (l1 > l0) ? l0 : W - l0;
        } else {
            ty = 0;
            wid = W;
        }
    };
    std::vector<int> on_simd[2]; // per (cu, simd): wavefront 0 / wavefront 1 member (grid wavefront index or -1)
    on_simd[0].assign((size_t)ncu * 4, -1);
    on_simd[1].assign((size_t)ncu * 4, -1);
    for (int W = 0; W < NW; ++W) {
        const int g = W / 2, j = W % 2, cu = g % ncu, pass = g / ncu, simd = (pass + j) % 4;
        on_simd[j][(size_t)cu * 4 + simd] = W;
    }
    std::vector<double> q((size_t)NW, 0.0);
    int npairs = 0;
    for (size_t k = 0; k < on_simd[0].size(); ++k) npairs += (on_simd[0][k] >= 0 && on_simd[1][k] >= 0);
    int ip = 0;
    for (size_t k = 0; k < on_simd[0].size(); ++k) {
        const int a = on_simd[0][k], b = on_simd[1][k];
        if (a >= 0 && b >= 0) {
            const double u = (ip + 0.5) / (2.0 * npairs);
            q[(size_t)((ip & 1) ? a : b)] = u;        // (alternating which member takes the long share spreads the long
            q[(size_t)((ip & 1) ? b : a)] = 1.0 - u;  //  models evenly over the two targets)
            ++ip;
        } else if (a >= 0) {
            q[(size_t)a] = 0.0;
        } else if (b >= 0) {
            q[(size_t)b] = 0.0;
        }
    }
    const int nw[2] = {n0, n1};
    for (int t = 0; t < 2; ++t) {
        std::vector<std::pair<double, int>> v;
        for (int W = 0; W < NW; ++W) {
            int ty, wid;
            target_of(W, ty, wid);
            if (ty == t && wid < nw[t] - 1) v.emplace_back(q[(size_t)W], wid); // (the last wavefront keeps the tail)
        }
        std::sort(v.begin(), v.end());
        rank[t].assign((size_t)(nw[t] > 0 ? nw[t] : 1), 0);
        for (size_t r = 0; r < v.size(); ++r) rank[t][(size_t)v[r].second] = (int32_t)r;
    }
    return true;
}

// Second launch of a call in BH_SEARCH_FAST: the models the guard fired on (per target: counts[t], lists + t * (B + 4)),
// again, with the reference's sequence -- one model per wavefront, as many trials per round as its lanes admit.  The launch
// is sized for the worst case and reads the counts on the device: workgroups beyond them leave at once (no host round trip;
// nearly always all of them).  Rows and failure flags of the listed models are overwritten with the reference's.
// sx: null, or the period table of the main launch (its targets are this launch's): the site-period build of the same name.
int launch_swd_rerun(bh_engine *e, hipStream_t st, const SwdMultiArgs &main, int32_t *counts, int32_t *lists, const SwdSiteXArgs *sx = nullptr)
{
    SwdMultiArgs a = main;
    a.rerun = 1;
    a.perm = nullptr;
    a.split = nullptr;
    a.Lcut = a.Lmax;
    a.started = nullptr;
    a.stamp = swd_stamp(e);
    a.adapt_ok = 1;
    SwdGroupAsk q{};
    q.B = a.B; q.Lmax = q.Lcut = a.Lmax; q.ntargets = a.ntargets;
    q.G0 = bh_swd_pick_group(a.B, a.ntargets, a.Lmax);
    for (int t = 0; t < a.ntargets; ++t) {
        SwdTarget &T = a.t[t];
        T.perm = lists + (size_t)t * (size_t)(a.B + 4);
        T.count = counts + t;
        T.gcount = nullptr;
        T.glist = nullptr;
        T.look = 64 / q.G0 > 1 ? 64 / q.G0 : 1; // one model per wavefront
        T.inlook = 1;
        q.t[t] = SwdGroupAsk::Target{T.K, T.look, T.iwave, T.mode, T.igr != 0, T.refseq != 0};
    }
    q.adapt_ok = q.rerun = true; q.counters = a.neval != nullptr; q.scan = e->swd_scan; q.sitex = sx != nullptr;
    const SwdGroupPlan g = bh_plan_swd_group(q, bh_tuning());
    if (!g.fits) return fail(e, BH_EINVAL, "model too deep for LDS");
    set_group_args(a, g);
    if (sx == nullptr) bh_launch_swd_group(a, g, st);
    else if (!bh_launch_swd_group_x(a, g, *sx, st)) return fail(e, BH_EUNSUPPORTED, "no site-period build of this dispersion launch");
    note_group(e, BH_SWD_RERUN, g, false);
    HIPCHK(e, hipGetLastError());
    ++e->rerun_launches;
    return BH_OK;
}

// The SIMD-pairing order (SwdPairWork) of the group kernel's launch c.g: c.pair_perm.  Placement tables are rebuilt when the
// launch's wavefront counts change; where they cannot be made the order is the plain sorted one, where work space cannot be
// allocated, or the launch is not one the order is defined for, the models keep the caller's order.
int pair_models(SwdCall &c)
{
    SwdPairWork &pw = c.e->pairwork;
    const SwdGroupPlan &g = c.g;
    const int nt = c.p.ntargets, B = c.m.B;
    const int *n = g.pair_waves;
    bool ok = g.pair, geom = true; // (not in a two-dimensional grid: the caller's order)
    if (ok && (pw.key_n0 != n[0] || pw.key_n1 != n[1])) { // (rare: the batch shape changed)
        std::vector<int32_t> rank[2];
        geom = build_slot_ranks(n[0], n[1], pw.ncu, rank); // false: placement unknown -> plain sorted order
        for (int t = 0; ok && geom && t < nt; ++t) {
            if (pw.cap_rank[t] < n[t]) {
                if (pw.slot_rank[t]) (void)hipFree(pw.slot_rank[t]);
                pw.slot_rank[t] = nullptr;
                ok = hipMalloc((void **)&pw.slot_rank[t], (size_t)(n[t] + 64) * sizeof(int32_t)) == hipSuccess;
                pw.cap_rank[t] = ok ? n[t] + 64 : 0;
            }
            if (ok) {
                ok = hipStreamSynchronize(c.st) == hipSuccess && // (an earlier launch may still read the old table)
                     hipMemcpy(pw.slot_rank[t], rank[t].data(), (size_t)n[t] * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess;
            }
        }
        pw.key_n0 = (ok && geom) ? n[0] : -1;
        pw.key_n1 = (ok && geom) ? n[1] : -1;
    }
    if (ok && pw.cap_perm < B) {
        for (int t = 0; t < 2; ++t) {
            if (pw.perm[t]) (void)hipFree(pw.perm[t]);
            pw.perm[t] = nullptr;
            ok = ok && hipStreamSynchronize(c.st) == hipSuccess &&
                 hipMalloc((void **)&pw.perm[t], (size_t)(B + B / 4 + 64) * sizeof(int32_t)) == hipSuccess;
        }
        pw.cap_perm = ok ? B + B / 4 + 64 : 0;
    }
    // (the launch is the call's prologue, SwdPlan::prologue: where there is no order to compute it still zeroes the fills)
    PairOrderTarget tg[2] = {};
    for (int t = 0; ok && t < nt; ++t) tg[t] = PairOrderTarget{g.pair_mpw[t], n[t], geom ? pw.slot_rank[t] : nullptr, pw.perm[t]};
    const SwdTarget t0 = swd_target(c, c.p.job[0]); // (its S velocities predict the search lengths: flattened for flsph = 1)
    c.order_wgs = bh_launch_pair_order(B, c.m.Lmax, c.m.nlay, t0.vs, t0.sl, t0.sb, ok ? nt : 0, tg, c.fills, c.st);
    for (int t = 0; ok && t < nt; ++t) c.pair_perm[t] = pw.perm[t];
    (void)hipGetLastError();
    return BH_OK;
}

// The order the plan asks for, computed on the device: c.perm (and c.split for two depth classes), or c.pair_perm.
int order_models(SwdCall &c)
{
    const SwdPlan &p = c.p;
    if (p.order == ORDER_NONE) return BH_OK;
    if (p.order == ORDER_PAIR) return pair_models(c);
    bh_engine *e = c.e;
    int rc;
    if ((rc = ensure(e, e->perm, ((size_t)c.m.B + 4) * sizeof(int32_t)))) return rc;
    int32_t *perm = (int32_t *)e->perm.p;
    if (p.order == ORDER_LENGTH) {
        const PairOrderTarget tg{p.len_mpw, c.m.B / p.len_mpw, nullptr, perm + 4, p.len_xcd};
        c.order_wgs = bh_launch_pair_order(c.m.B, c.m.Lmax, c.m.nlay, c.m.vs, c.m.sl, c.m.sb, 1, &tg, c.fills, c.st);
    } else {
        bh_launch_order(c.m.B, c.m.nlay, perm + 4, p.Lcut, perm, c.st);
        c.order_wgs = 1;
        c.split = (p.Lcut < c.m.Lmax) ? perm : nullptr;
    }
    c.perm = perm + 4;
    return BH_OK;
}

// One lane per model: a launch per target.  A wavefront of these kernels keeps its SIMD's vector issue ~60 % busy
// (profiles/), so the targets of a call run SIDE BY SIDE: every second one on a second stream.  ra: the targets for the
// re-run of guarded models (which goes through the group kernel).
int launch_swd_lanes(SwdCall &c, SwdMultiArgs &ra)
{
    bh_engine *e = c.e;
    const SwdPlan &p = c.p;
    const int B = c.m.B, n = p.ntargets;
    const bool fork = n > 1 && e->aux2 != nullptr;
    int rc;
    // work array of the launches (the Neville orders the kernel does not keep in LDS): one region per target,
    // the targets run concurrently
    size_t nev_off[BH_MAX_TARGETS + 1] = {0};
    for (int t = 0; t < n; ++t) nev_off[t + 1] = nev_off[t] + bh_swd_nev_high_doubles(B, p.look[t]);
    if ((rc = ensure(e, e->nevhi, nev_off[n] * sizeof(double)))) return rc;
    long lane_waves = 0; // wavefronts of the call
    for (int t = 0; t < n; ++t) lane_waves += (long)((B + 63) / 64) * p.look[t];
    e->guard_last = p.any_fast;
    ra.B = B; ra.Lmax = c.m.Lmax; ra.nlay = c.m.nlay; ra.neval = c.counter; ra.counted = e->swd_scan;
    if (p.any_fast && (rc = swd_board(e, c.st, &ra.board))) return rc;
    e->last_swd_kernel = BH_KERNEL_LANE;
    ev_begin(e, 0, c.st);
    if (fork && (rc = wait_for(e, e->ev_fork2, c.st, e->aux2))) return rc;
    for (int t = 0; t < n; ++t) {
        const SwdTarget tg = swd_target(c, p.job[t]);
        SwdKernelArgs a = lane_args(c, tg);
        a.look = p.look[t];
        // priority time slice (log2 cycles) of wavefronts that share a SIMD, see swd_kernel; wavefronts with a SIMD of
        // their own are left alone (a low-priority phase costs them 8 %: the CU's front end is shared)
        a.fair = lane_waves <= 1024 ? -1 : (lane_waves <= 2048 ? 18 : 12);
        a.nev_high = (double *)e->nevhi.p + nev_off[t];
        a.fast = p.fast[t] ? 1 : 0;
        a.farith = (p.fast[t] && p.farith) ? 1 : 0;
        if (a.fast) {
            a.gcount = c.gcounts + t;
            a.glist = c.glists + (size_t)t * (size_t)(B + 4);
        }
        SwdLaneBuild lb{};
        bh_launch_swd(a, tg.iwave, (fork && (t & 1)) ? e->aux2 : c.st, &lb);
        note_lane(e, BH_SWD_MAIN, lb);
        ra.t[ra.ntargets++] = tg;
    }
    if (fork && (rc = wait_for(e, e->ev_join2, e->aux2, c.st))) return rc;
    HIPCHK(e, hipGetLastError());
    return BH_OK;
}

// All targets in ONE launch of the group kernel (G lanes per model) or of the trial-per-lane kernel.  a: the launch's arguments
// (what the re-run of guarded models starts from).
int launch_swd_multi(SwdCall &c, SwdMultiArgs &a)
{
    bh_engine *e = c.e;
    const SwdPlan &p = c.p;
    const int B = c.m.B;
    int rc;
    if ((rc = swd_board(e, c.st, &a.board))) return rc;
    a.stamp = swd_stamp(e);
    a.B = B; a.Lmax = c.m.Lmax; a.nlay = c.m.nlay; a.neval = c.counter; a.perm = c.perm;
    a.split = c.split; a.Lcut = p.Lcut;
    a.ntargets = p.ntargets;
    for (int t = 0; t < p.ntargets; ++t) {
        a.t[t] = swd_target(c, p.job[t]);
        a.t[t].look = p.look[t];
        a.t[t].inlook = p.inlook[t];
        a.t[t].refseq = p.refseq[t] ? 1 : 0;
    }
    a.started = e->started;
    a.prio_low = c.prio_low;
    a.adapt_ok = p.adapt_ok ? 1 : 0;
    if (p.sitex) { // the period table with this launch's targets
        c.sx = *c.jobs[p.job[0]].sx.tab;
        for (int t = 0; t < p.ntargets; ++t) {
            c.sx.col[t] = c.jobs[p.job[t]].sx.col;
            c.sx.off[t] = c.jobs[p.job[t]].sx.off;
        }
    }
    const bool lean = p.kernel == BH_KERNEL_LEAN;
    if (lean) {
        a.counted = e->swd_scan;
        a.farith = p.farith ? 1 : 0;
        a.fast = p.any_fast ? 1 : 0;
        // Issue priority shared out by the clock (swd_lean_kernel) where the dispatcher is known to put one Rayleigh and one
        // Love wavefront on every SIMD: two targets with the same wavefront count in workgroups of four, more than one and at most
        // two workgroups per CU (the second pass sits one SIMD on, build_slot_ranks).  Every other launch: as dispatched.
        // Exactly two workgroups per CU (c2 at B = 4096 on 256 CUs): which positions share a SIMD is known too (lean_half), and
        // the Love wavefront beside the Rayleigh wavefront of rank r takes the Love group of the opposite rank.
        a.lean_prio = a.lean_half = 0;
        const BhTuning &tun = bh_tuning();
        if (p.ntargets == 2 && p.look[0] == 16 && p.look[1] == 16 && !p.sitex && a.t[0].iwave != a.t[1].iwave) { // (the build: swd_lean_kernel<16, ., true>)
            const int mpw = BH_WAVE / p.look[0];
            const long waves = 2L * ((B + mpw - 1) / mpw), wgs = (waves + 3) / 4, ncu = e->pairwork.ncu;
            if (ncu > 0 && wgs > ncu && wgs <= 2 * ncu && waves % 4 == 0) {
                const int slice = tun.swd_lean_slice >= 8 && tun.swd_lean_slice <= 24 ? tun.swd_lean_slice : LEAN_PRIO_SLICE;
                if (tun.swd_lean_share > 0 && tun.swd_lean_share <= 8) a.lean_prio = tun.swd_lean_share | (slice << 8);
                if (wgs == 2 * ncu && ncu % 32 == 0 && tun.swd_lean_no_half == 0) a.lean_half = (int)(ncu / 4);
            }
        }
    } else {
        for (int t = 0; t < 2; ++t) a.t[t].perm = c.pair_perm[t];
        set_group_args(a, c.g);
    }
    if (bh_tuning().debug_plan != 0) {
        std::fprintf(stderr, "[bh] dispersion plan B=%d Lmax=%d: lanes per model %d, typical layers %d (hint %d), Lcut %d%s, pairing %d; trials per round:",
                     B, c.m.Lmax, p.G, c.m.typ_layers, e->hint_layers, p.Lcut, p.Lcut < c.m.Lmax ? " (two depth classes)" : "", (int)(p.order == ORDER_PAIR));
        for (int t = 0; t < p.ntargets; ++t) std::fprintf(stderr, " %s %d/%d", a.t[t].iwave == BH_WAVE_LOVE ? "L" : "R", p.look_group[t], p.inlook[t]);
        if (!lean) std::fprintf(stderr, "; launched lanes per model %d/%d", c.g.lanes[0], c.g.lanes[1]);
        std::fprintf(stderr, "\n");
    }
    e->guard_last = p.any_fast;
    if (p.any_fast) {
        for (int t = 0; t < a.ntargets; ++t)
            if (a.t[t].igr == BH_VEL_PHASE) {
                a.t[t].gcount = c.gcounts + t;
                a.t[t].glist = c.glists + (size_t)t * (size_t)(B + 4);
            }
    }
    ev_begin(e, 0, c.st);
    e->last_swd_kernel = p.kernel;
    if (lean) {
        SwdLaneBuild lb{};
        if ((p.sitex ? bh_launch_swd_lean_x(a, c.sx, c.st, &c.info, &lb) : bh_launch_swd_lean(a, c.st, &c.info, &lb)) != 0)
            return fail(e, BH_EINVAL, "model too deep for LDS");
        note_launch(e, BH_KERNEL_LEAN, BH_SWD_MAIN, lb.key, false, p.ntargets == 2, false, false, lb.grid_x, a.lean_prio >> 8);
    } else {
        if (!p.sitex) bh_launch_swd_group(a, c.g, c.st);
        else if (!bh_launch_swd_group_x(a, c.g, c.sx, c.st)) return fail(e, BH_EUNSUPPORTED, "no site-period build of this dispersion launch");
        note_group(e, BH_SWD_MAIN, c.g, c.pair_perm[0] != nullptr);
        c.info = c.g.info;
    }
    // (the counter a second stream waits on moves only once the launch is known to have been accepted: a failed launch
    // never increments the device word, and every later wait for the advanced value would hang -- ADVICE r03)
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return fail(e, BH_EHIP, "dispersion kernel launch", le);
    if (e->started) e->started_expected += c.info.workgroups;
    return BH_OK;
}

// The second roots of the group-velocity targets split in two launches (plan_swd): B x K independent searches per target,
// after the call's other launches.  Each search reads the first root its chain kept and puts the group velocity in its place.
// Periods per site on such a target (bh_sites_set_x_all): K is the capacity of the target's columns -- the host does not know the
// sites of a device-resident call, so lanes and work space are sized for B x capacity entries -- and the launch is the
// site-period build's (bh_launch_swd_second_x), with the main launch's period table: an entry beyond its site's count is idle.
int launch_second_roots(const SwdCall &c)
{
    bh_engine *e = c.e;
    const int B = c.m.B;
    int J2 = 16; // trial lanes per search while all searches of the call still fit the chip at once (2048 wavefronts)
    {
        long searches = 0;
        for (int t = 0; t < c.p.ntargets; ++t) searches += c.p.first_roots[c.p.job[t]] ? (long)B * c.jobs[c.p.job[t]].K : 0;
        while (J2 > 1 && searches * J2 > 2048L * 64) J2 >>= 1;
    }
    size_t off[BH_MAX_TARGETS + 1] = {0};
    int n = 0;
    for (int t = 0; t < c.p.ntargets; ++t)
        if (c.p.first_roots[c.p.job[t]]) {
            off[n + 1] = off[n] + bh_swd_nev_high_doubles(B * c.jobs[c.p.job[t]].K, J2);
            ++n;
        }
    int rc = ensure(e, e->nevhi2, off[n] * sizeof(double));
    if (rc) return rc;
    // (as with the one-lane-per-model launches: every second target on a second stream, side by side)
    const bool fork = n > 1 && e->aux2 != nullptr;
    if (fork && (rc = wait_for(e, e->ev_fork2, c.st, e->aux2))) return rc;
    n = 0;
    for (int t = 0; t < c.p.ntargets; ++t) {
        if (!c.p.first_roots[c.p.job[t]]) continue;
        const SwdTarget tg = swd_target(c, c.p.job[t]);
        SwdKernelArgs a = lane_args(c, tg);
        a.B = B * tg.K; a.Bm = B; a.second = 1;
        a.igr = BH_VEL_GROUP; a.mode = 1; a.perm = nullptr;
        a.look = J2;
        const long waves = ((long)a.B * J2 + 63) / 64;
        a.fair = waves <= 1024 ? -1 : (waves <= 2048 ? 18 : 12);
        a.nev_high = (double *)e->nevhi2.p + off[n];
        SwdLaneBuild lb{};
        const SwdSiteJob &sx = c.jobs[c.p.job[t]].sx;
        if (sx.tab != nullptr && sx.all) bh_launch_swd_second_x(a, tg.iwave, c.sx, t, (fork && (n & 1)) ? e->aux2 : c.st, &lb);
        else bh_launch_swd(a, tg.iwave, (fork && (n & 1)) ? e->aux2 : c.st, &lb);
        note_lane(e, BH_SWD_SECOND, lb);
        ++n;
    }
    if (fork && (rc = wait_for(e, e->ev_join2, e->aux2, c.st))) return rc;
    HIPCHK(e, hipGetLastError());
    return BH_OK;
}

} // namespace

namespace bheng {

// igr: 0 is a phase velocity; any value > 0 a group velocity (surfdisp96.f:77, :232, :282), normalised here to BH_VEL_GROUP
int swd_supported(bh_engine *e, int K, int iwave, int &igr, int mode, int flsph)
{
    if (K < 0 || K > BH_MAX_PERIODS) return fail(e, BH_EINVAL, "K must be 0..60 (surfdisp96.f:61-62)");
    if (iwave != BH_WAVE_LOVE && iwave != BH_WAVE_RAYLEIGH) return fail(e, BH_EINVAL, "iwave must be 1 (Love) or 2 (Rayleigh)");
    if (igr < 0) return fail(e, BH_EINVAL, "igr must be 0 (phase velocity) or > 0 (group velocity)");
    if (mode < 1 || mode > 16) return fail(e, BH_EINVAL, "mode must be 1..16");
    if (flsph != 0 && flsph != 1) return fail(e, BH_EINVAL, "flsph must be 0 or 1");
    igr = igr > 0 ? BH_VEL_GROUP : BH_VEL_PHASE;
    return BH_OK;
}

// stream `to` waits for what `from` has enqueued so far: the fork to and the join from the engine's second stream, on which
// every second launch of a call runs side by side with the others
int wait_for(bh_engine *e, hipEvent_t ev, hipStream_t from, hipStream_t to)
{
    HIPCHK(e, hipEventRecord(ev, from));
    HIPCHK(e, hipStreamWaitEvent(to, ev, 0));
    return BH_OK;
}

// The plan of a call's dispersion jobs on the staged batch m (no dispersion job: a plan without targets, order or prologue)
SwdPlan plan_swd_call(const bh_engine *e, const ModelBatch &m, int njobs, const SwdJob *jobs)
{
    return plan_swd(e, m.B, m.Lmax, m.typ_layers > 0 ? m.typ_layers : e->hint_layers, njobs, jobs);
}

// All dispersion targets of one call: the plan, the flattened copies and the order it needs, then its launches -- the group or
// trial-per-lane kernel (one launch for all targets) or one lane per model (a launch per target) -- the re-run of the models
// the guard of the short refinement fired on, and the second roots of split group velocities.
// p: the call's plan (plan_swd_call).  fills: where p.prologue, what the caller leaves to the ordering launch to zero (the guard's
// head and the counters are added here).  prio_low: SwdMultiArgs::prio_low of the main launch.  main: null, or where the
// SwdLaunchInfo of the call's main launch goes once the call has dispersion targets (workgroups == 0: not a launch of the group
// or trial-per-lane kernel).
int launch_swd_jobs(bh_engine *e, hipStream_t st, const ModelBatch &m, int njobs, const SwdJob *jobs, const SwdPlan &p,
                    const SwdFills &fills, int prio_low, SwdLaunchInfo *main)
{
    const int B = m.B, Lmax = m.Lmax;
    if (B == 0 || njobs == 0) return BH_OK;
    SwdCall c{e, st, m, jobs, p};
    c.prio_low = prio_low;
    c.fills = fills;
    if (p.kernel == BH_KERNEL_GROUP) {
        c.g = plan_group(e, p, B, Lmax, jobs);
        if (!c.g.fits) return fail(e, BH_EINVAL, "model too deep for LDS");
    }
    int rc;
    if (p.nsplit > 0) {
        if ((rc = ensure(e, e->gfirst, (size_t)p.nsplit * B * sizeof(double)))) return rc;
        int n = 0;
        for (int j = 0; j < njobs; ++j)
            if (p.first_roots[j]) c.first[j] = (double *)e->gfirst.p + (size_t)(n++) * B;
    }
    if (p.ntargets == 0) return BH_OK;
    e->n_swd_launches = 0; // (bh_engine_last_swd_launches: this call's)
    if (p.any_sphere) { // earth-flattened copies of the batch (layer-major), made once per call
        const size_t ne = (size_t)Lmax * B;
        if ((rc = ensure(e, e->sph, 5 * ne * sizeof(double)))) return rc;
        double *base = (double *)e->sph.p;
        bh_launch_sphere(B, Lmax, m.nlay, m.h, m.vp, m.vs, m.rho, m.sl, m.sb, base, base + ne, base + 2 * ne, base + 3 * ne, base + 4 * ne, st);
        c.sph = base;
    }
    // the call's fills: the ordering launch's where the plan has one (SwdPlan::prologue), else dispatches of their own
    SwdFills *const prologue = p.prologue ? &c.fills : nullptr;
    if ((rc = swd_counter(e, st, prologue, &c.counter))) return rc;
    if (p.any_fast && (rc = guard_space(e, st, B, prologue, &c.gcounts, &c.glists))) return rc;
    if ((rc = order_models(c))) return rc;
    e->last_swd_order[0] = p.order;
    for (int t = 0; t < 2; ++t) e->last_swd_perm[t] = p.order == ORDER_NONE ? nullptr : (c.pair_perm[t] != nullptr ? c.pair_perm[t] : c.perm);
    e->last_swd_perm_n = B;
    e->last_swd_order[1] = c.order_wgs;
    e->last_swd_order[2] = !p.prologue ? 0 : (c.fills.nguard > 0 ? BH_FILL_GUARD : 0) | (c.fills.nerr > 0 ? BH_FILL_FLAGS : 0) | (c.fills.ncounter > 0 ? BH_FILL_COUNTERS : 0);
    SwdMultiArgs a{};
    rc = p.kernel == BH_KERNEL_LANE ? launch_swd_lanes(c, a) : launch_swd_multi(c, a);
    if (main) *main = c.info;
    // (guarded models of the short refinement: re-run, unless the group kernel restarts them in place)
    if (!rc && p.any_fast && !(p.kernel == BH_KERNEL_GROUP && c.g.restart)) rc = launch_swd_rerun(e, st, a, c.gcounts, c.glists, p.sitex ? &c.sx : nullptr);
    if (!rc && p.nsplit > 0) rc = launch_second_roots(c);
    ev_end(e, 0, st);
    return rc;
}

} // namespace bheng

extern "C" {

int bh_swd_batch(bh_engine *e, int memspace, void *stream, int B, int Lmax, const int32_t *nlay,
                 const double *h, const double *vp, const double *vs, const double *rho,
                 ptrdiff_t sl, ptrdiff_t sb, int K, const double *periods, int iwave, int igr,
                 int mode, int flsph, double *vel, int32_t *err)
{
    int rc;
    ModelBatch m{B, Lmax, nlay, h, vp, vs, rho, nullptr, nullptr, sl, sb};
    if ((rc = check_models(e, m))) return rc;
    if ((rc = swd_supported(e, K, iwave, igr, mode, flsph))) return rc;
    if (!nlay || !h || !vp || !vs || !rho || !periods || !vel || !err) return fail(e, BH_EINVAL, "null argument");
    if (B == 0) return BH_OK;
    HIPCHK(e, hipSetDevice(e->device));
    const bool host = (memspace != BH_DEVICE);
    hipStream_t st = (!host && stream) ? (hipStream_t)stream : e->stream;
    SwdJob job{K, iwave, igr, K, periods, vel, err, mode, flsph};
    if (host) {
        if ((rc = stage_models(e, m))) return rc;
        if ((rc = ensure(e, e->periods, (size_t)BH_MAX_PERIODS * sizeof(double)))) return rc;
        if ((rc = ensure(e, e->vel, (size_t)B * K * sizeof(double)))) return rc;
        if ((rc = ensure(e, e->errb, (size_t)B * sizeof(int32_t)))) return rc;
        HIPCHK(e, hipMemcpyAsync(e->periods.p, periods, (size_t)K * sizeof(double), hipMemcpyHostToDevice, st));
        job.periods_dev = (const double *)e->periods.p; job.vel = (double *)e->vel.p; job.err = (int32_t *)e->errb.p;
    }
    call_begin(e, st);
    rc = launch_swd_jobs(e, st, m, 1, &job, plan_swd_call(e, m, 1, &job), SwdFills{}, 0, nullptr);
    call_end(e, st);
    if (rc || !host) return rc;
    HIPCHK(e, hipMemcpyAsync(vel, e->vel.p, (size_t)B * K * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipMemcpyAsync(err, e->errb.p, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    return BH_OK;
}

} // extern "C"
