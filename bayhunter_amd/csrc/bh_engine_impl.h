// bayhunter_amd/csrc/bh_engine_impl.h -- what the engine's four host units share (bh_engine.hip, engine_swd.hip, engine_register.hip,
// engine_eval.hip) and nothing else includes: the engine's state and its site table, the error and buffer helpers, the model batch of
// a call, the registration's upload step, and the declarations of the few functions that cross units.  Host code only; everything
// but struct bh_engine (the C ABI's opaque handle) is in namespace bheng.
#ifndef BH_ENGINE_IMPL_H
#define BH_ENGINE_IMPL_H

#include "../../include/bh_engine_debug.h"
#include "../../include/bh_engine_sites.h"
#include "../../include/bh_engine_sites_rf.h"
#include "../../include/bh_engine_sites_x.h"
#include "../../include/bh_engine_sites_x_all.h"
#include "../../include/bh_engine_sites_missing.h"
#include "../../include/bh_engine_sites_gauss.h"
#include "../../include/bh_engine_sites_rf_axis.h"
#include "../../include/bh_engine_sites_laws.h"
#include "../../include/bh_engine_ellip_target.h"
#include "../../include/bh_engine_sites_ellip.h"
#include "bh_device.h"
#include "bh_tuning.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

namespace bheng {

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

struct TargetHost {
    bh_target_desc d{};
    int off = 0; // column offset in a ymod row
    DevBuf x, yobs, yerr_scaled, rinv, quad;
    DevBuf sums;       // receiver function, fused likelihood (EvalPlan::rf_fused): [B][4] sums of the call (RfKernelArgs::sums)
    DevBuf x60, vel60; // > 60 periods: the 60-point grid the forward model runs on + its output
    int kfwd = 0;      // periods the forward model computes (n, or 60 when n > 60)
    double logdet_extra = 0.0;
    // what the plan of an ellipticity target compares (bh_plan_ellip): the periods of a dispersion or ellipticity target as
    // registered, and an id of their bit pattern among the registered targets (equal ids = equal bits; -1: none)
    std::vector<double> x_host;
    int xid = -1;
    // BH_TARGET_ELLIP (bh_targets_set_ellip): the polish steps and the transform; the velocities of a search of its own
    int ell_nsteps = 0, ell_signed = 0, ell_zh = 0;
    DevBuf ell_vel;    // [B][n]
    bool ell_sites = false; // bh_targets_set_ellip_sites: periods and counts per site, from the count table (n: the capacity)
};

inline void release(DevBuf &b)
{
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}

// ---- the site table: everything the bh_sites_set* entry points register for the targets of bh_targets_set ----
// What the tables in force say of one registered target
struct SiteTarget {
    bool lacks = false;            // the count table has a site with count 0 for this target
    bool rf_own_counts = false;    // receiver function: the count table (bh_sites_set_axes) has a count that is neither 0 nor the descriptor's
    bool law_other = false;        // the law table has a present site under another law than BH_LAW_GAUSS (read for a Gauss-law target)
    int axis_nsamp_max = 0;        // receiver function: the largest nsamp of the column of bh_sites_set_rf_axis
    int nclass = 0;                // correlation classes of a Gauss-law target (bh_sites_set_gauss); 0: none, every site takes the descriptor's matrix
    DevBuf rinv, logdet, class_of; // [nclass][n][n], [nclass], int32 [nsites]
};

// The parts of the table, each registered on top of the one before it
enum SitePart { PART_COUNTS, PART_RF, PART_RF_AXIS, PART_LAWS, PART_CLASSES };

struct SiteTable {
    SiteLevel level = SITES_NONE;   // what the counts (bh_sites_set, bh_sites_set_x ... bh_sites_set_axes) let the sites differ in
    int nsites = 0;
    DevBuf yobs, yerr, logdet;      // observed data: [nsites][ldy], [nsites][ldy] (law-1 columns), [nsites][nt]
    DevBuf idx;                     // host calls: the site index of every model, staged
    DevBuf xn, xper;                // level >= SITES_X: [nsites][nt] sample counts (int32), [nsites][ldy] periods in ymod's column layout
    std::vector<int32_t> xn_host;   // ... the counts as registered (the later parts are checked against them)
    bool rf = false;                // receiver-function parameters per site (bh_sites_set_rf) are in force
    DevBuf p, nsv;                  // [nsites][nt]: p (s/deg) and nsv of every site, read in the RF columns only
    bool rf_axis = false;           // receiver-function time axis and Gauss filter per site (bh_sites_set_rf_axis) are in force
    DevBuf axis;                    // [nsites][nt] RfAxisRec, read in the RF columns only
    bool laws = false;              // noise law per site (bh_sites_set_laws) is in force
    DevBuf law, law_yerr, law_logdet; // int32 [nsites][nt] (0 where the count is 0); the law-1 tables by the TABLE's law: [nsites][ldy], [nsites][nt]
    std::vector<int32_t> law_host;  // ... the laws as registered (bh_sites_set_gauss checks its classes against them)
    DevBuf desc_n;                  // [nsites][nt] the descriptors' counts: the count table of a class call below SITES_X
    DevBuf class_work;              // the grouping's work space of a call (bh_gauss_class_work_words)
    int32_t ell_source[BH_MAX_TARGETS] = {}; // level >= SITES_X_ALL: bh_plan_ellip_sites of the count table as registered (plan_eval reads it)
    SiteTarget t[BH_MAX_TARGETS];

    // The one invalidation rule.  `part` is being registered anew -- out of force until its entry point has succeeded -- and what
    // was registered on top of it goes with it:
    //     counts (the shared table of bh_sites_set included)   drop   rf, axis, laws, classes: everything
    //     rf                                                   drops  axis, laws, classes
    //     axis                                                 drops  laws, classes
    //     laws                                                 drop   classes (they were checked against the laws)
    //     classes of target `target`                           drop   nothing else
    // Every line down to the laws is the line below it and one part more: those cases fall through.  The table belongs to the
    // registered targets: bh_targets_set and bh_engine_destroy drop it as a whole.
    void drop(SitePart part, int target = -1)
    {
        switch (part) {
        case PART_COUNTS:
            for (DevBuf *b : {&yobs, &yerr, &logdet, &idx, &xn, &xper, &p, &nsv, &axis}) release(*b);
            level = SITES_NONE;
            nsites = 0;
            xn_host.clear();
            for (SiteTarget &T : t) T.lacks = T.rf_own_counts = false;
            for (int32_t &j : ell_source) j = -1;
            [[fallthrough]];
        case PART_RF:
            rf = false;
            [[fallthrough]];
        case PART_RF_AXIS:
            rf_axis = false;
            for (SiteTarget &T : t) T.axis_nsamp_max = 0;
            [[fallthrough]];
        case PART_LAWS:
            for (DevBuf *b : {&law, &law_yerr, &law_logdet}) release(*b);
            laws = false;
            law_host.clear();
            for (SiteTarget &T : t) T.law_other = false;
            for (SiteTarget &T : t) {
                for (DevBuf *b : {&T.rinv, &T.logdet, &T.class_of}) release(*b);
                T.nclass = 0;
            }
            release(desc_n);
            break;
        case PART_CLASSES: // (of one target; its buffers serve the registration that follows)
            t[target].nclass = 0;
        }
    }
};

} // namespace bheng

struct bh_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t aux = nullptr;             // receiver-function kernels run here, next to the dispersion kernel
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipStream_t aux2 = nullptr;            // second dispersion target of a lane-per-model call runs here, beside the first
    hipEvent_t ev_fork2 = nullptr, ev_join2 = nullptr;
    bool overlap_rf = true;                // BH_NO_OVERLAP env turns it off (A/B testing)
    int rf_lds_beside_swd = 40 * 1024;     // BH_RF_LDS_BESIDE env (bytes; experiment switch), see bh_plan_rf
    // co-resident receiver function (the start gate: plan_eval, gate_need): the dispersion kernel counts its started workgroups here
    unsigned *started = nullptr;           // device word (signal memory where available), cumulative over launches
    unsigned started_expected = 0;         // value after every launch enqueued so far has started
    int swd_prio_low = 1;                  // BH_SWD_PRIO_LOW env: dispersion wavefronts' low priority while RF wavefronts run beside them
    SwdPairWork pairwork{};                // SIMD-pairing order of the group kernel (bh_device.h)
    int swd_trials = 0;                    // bh_engine_set_swd_trials: trials per round of the trial-per-lane kernel (0 = by the call's shape)
    int last_swd_kernel = -1;              // bh_engine_last_swd_kernel
    bh_swd_launch swd_launches[3 * BH_MAX_TARGETS]{}; // bh_engine_last_swd_launches: of the most recent call with dispersion targets
    int n_swd_launches = 0;
    const int32_t *last_swd_perm[2] = {nullptr, nullptr}; int last_swd_perm_n = 0; // bh_engine_last_swd_perm: what the ordering launch wrote (device)
    int last_swd_order[3] = {0, 0, 0};     // bh_engine_last_swd_order: the plan's order, the ordering launch's workgroups, its fills
    int err_t_nt = -1, err_t_B = -1;       // layout for which err_t's untouched rows are known to be zero
    std::string err;
    // staging / workspace
    bheng::DevBuf nlay, h, vp, vs, rho, qp, qs, periods, vel, errb, rf, coef, ymod, noise, logL,
        misfits, err_t, probe_in, probe_out, counter, sph, perm, board, nevhi, rfz, gfirst, nevhi2;
    unsigned swd_stamp = 0;                // launch counter of the group kernel (marks its progress-board entries)
    // targets
    int nt = 0;
    int ldy = 0;
    std::vector<bheng::TargetHost> targets;
    bheng::SiteTable sites;                       // what the bh_sites_set* entry points registered for them
    // instrumentation
    bool timing = false, counting = false;
    bool no_mfma = false; // BH_NO_MFMA env: Gauss law through the in-kernel mat-vec (A/B testing)
    bool as_given = false; // bh_engine_set_model_order(e, 0): the caller's batches need no sorting by depth
    int force_group = 0; // BH_SWD_GROUP env / bh_engine_set_swd_group: 0 = choose automatically
    int force_look = 0;  // BH_SWD_LOOKAHEAD env / bh_engine_set_swd_lookahead: 0 = choose automatically
    int hint_layers = 0; // bh_engine_set_typical_layers: typical layer count of device-resident batches
    int swd_search = BH_SEARCH_FAST;  // bh_engine_set_swd_search / BH_SWD_SEARCH=reference|fast|fast_rayleigh: the short refinement (with its guard) for fundamental-mode phase-velocity targets unless told otherwise
    int swd_arith = BH_ARITH_FAST; // bh_engine_set_swd_arith / BH_SWD_ARITH=exact|fast: fast arithmetic in launches where every target takes the short refinement
    int swd_scan = 2;    // bh_engine_set_swd_scan / BH_SWD_SCAN=steps|counted|auto: Love scans skip the steps a mode count proves empty (same bits)
    bheng::DevBuf guard;        // short refinement: per target a count and a list of the models its guard fired on (re-run, see launch_swd_rerun)
    uint64_t rerun_launches = 0; // re-run launches enqueued so far (statistics)
    uint64_t guard_total[BH_MAX_TARGETS] = {0}; // guarded models of retired buffers (the live buffer carries its own running sum)
    bool guard_fresh = true;     // the guard buffer is new: zero its cumulative words as well
    bool guard_last = false;     // the most recent dispersion call had targets with the short refinement (its counts are in the buffer)
    // one EventSet per timed *_batch call since the last bh_timing_reset()
    struct EventSet {
        hipEvent_t ev[8];
        bool used[4];
    };
    std::vector<EventSet> evsets; // pool (events are reused after a reset)
    size_t ncalls = 0;            // sets in use
    uint64_t last_neval = 0;
    bool neval_pending = false;
};

namespace bheng {

// ---- errors and the engine's device buffers (bh_engine.hip) ----
// the engine's last error becomes `what` (with the HIP error's text behind it); returns code
int fail(bh_engine *e, int code, const char *what, hipError_t he = hipSuccess);

#define HIPCHK(e, call)                                                  \
    do {                                                                 \
        hipError_t _he = (call);                                         \
        if (_he != hipSuccess) return fail((e), BH_EHIP, #call, _he);    \
    } while (0)

// b holds at least `bytes` afterwards; a buffer that grows is a new one (the engine's streams are drained first), its content gone
int ensure(bh_engine *e, DevBuf &b, size_t bytes);

// The one registration step: b holds a copy of the `bytes` at src when it returns BH_OK (synchronous, as every registration is)
inline int upload(bh_engine *e, DevBuf &b, const void *src, size_t bytes, const char *what)
{
    if (int rc = ensure(e, b, bytes)) return rc;
    const hipError_t he = hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice);
    return he != hipSuccess ? fail(e, BH_EHIP, what, he) : BH_OK;
}

// every device buffer a registered target owns
inline void release_target(TargetHost &t)
{
    for (DevBuf *b : {&t.x, &t.yobs, &t.yerr_scaled, &t.rinv, &t.quad, &t.sums, &t.x60, &t.vel60, &t.ell_vel}) release(*b);
}

// Targets.py:124-128, the nocorr_scalederr law: out = yerr / min(yerr), returns ln prod(out) (bh_targets_set, bh_sites_set)
inline double scaled_errors(const double *yerr, int n, double *out)
{
    double mn = yerr[0];
    for (int i = 0; i < n; ++i) mn = yerr[i] < mn ? yerr[i] : mn;
    double prod = 1.0;
    for (int i = 0; i < n; ++i) {
        out[i] = yerr[i] / mn;
        prod *= out[i];
    }
    return std::log(prod);
}

// ---- the model arrays of one call ----
// B models in strided [Lmax][B] views (strides in elements, positive): the caller's arrays, or -- a BH_HOST call, once stage_models
// has run -- the engine's staging buffers.  rho, qp and qs may be null.
struct ModelBatch {
    int B, Lmax;
    const int32_t *nlay;
    const double *h, *vp, *vs, *rho, *qp, *qs;
    ptrdiff_t sl, sb;
    int typ_layers = 0; // typical layer count of the batch when the host can see it (0 = unknown)
};

// number of elements spanned by a view of the batch
inline size_t span_elems(const ModelBatch &m)
{
    return (size_t)((ptrdiff_t)(m.Lmax - 1) * m.sl + (ptrdiff_t)(m.B - 1) * m.sb + 1);
}

int check_models(bh_engine *e, const ModelBatch &m); // (bh_engine.hip)
int stage_models(bh_engine *e, ModelBatch &m);

// ---- the events of a timed call (bh_engine.hip; fam: 0 dispersion, 1 receiver function, 2 likelihood) ----
void ev_begin(bh_engine *e, int fam, hipStream_t st);
void ev_end(bh_engine *e, int fam, hipStream_t st);
void call_begin(bh_engine *e, hipStream_t st);
void call_end(bh_engine *e, hipStream_t st);

// ---- one dispersion call (engine_swd.hip) as the fused call (engine_eval.hip) and the registration see it ----
constexpr int GUARD_HEAD = 24; // words at the head of the guard's work space (guard_space), in front of the targets' lists

// The optional site arguments of a dispersion job: the periods and their count come from the model's site (SwdSiteXArgs), the
// job's K is the capacity of its output columns and periods_dev is not read.  tab: null = the job's own periods.
struct SwdSiteJob {
    const SwdSiteXArgs *tab; // the call's table (site, nsites, strides, n, x); col / off filled per launch
    int col, off;            // the job's registered target and its column offset in a row of x
    bool all;                // the table holds the periods of group-velocity targets as well (SitePlan::x_all): their second roots read it
};

struct SwdJob {
    int K, iwave, igr, ldv; // igr: BH_VEL_PHASE or BH_VEL_GROUP (swd_supported)
    const double *periods_dev;
    double *vel;
    int32_t *err;
    int mode = 1;
    int flsph = 0;
    SwdSiteJob sx{}; // periods per site (bh_evaluate_sites with a table of bh_sites_set_x)
};

// What the launches of one dispersion call do.  The call's targets are its jobs with K > 0, in job order.
struct SwdPlan {
    bool first_roots[BH_MAX_TARGETS]; // per job: the chain of first roots of a group velocity split in two launches
    int nsplit;                        // jobs that are
    int ntargets, kmax, maxmode;
    bool any_sphere;
    int typ_layers;                    // typical depth the lanes per model were chosen for (0: unknown, or ignored)
    int kernel;                        // BH_KERNEL_LEAN / GROUP / LANE
    int G, lean_trials;                // lanes per model; trials per round of the trial-per-lane kernel (>= 4: it runs)
    int order, Lcut;                   // SwdOrder; Lcut < Lmax: two depth classes
    bool prologue;                     // an ordering launch of bh_launch_pair_order precedes the dispersion launch: IT zeroes the guard's
                                       // head, the failure flags and the counters (SwdFills) and nothing else of the call fills them;
                                       // false: guard_space, run_forward and swd_counter enqueue their own fills
    int len_mpw, len_xcd;              // ORDER_LENGTH: models per wavefront and wavefronts per workgroup of the XCD blocks (0: none)
    bool sitex;                        // periods per model (SwdSiteJob): LDS rows of periods per model, no one-lane-per-evaluation kernel
    bool any_fast, farith, adapt_ok;   // some target takes the short refinement; its fast arithmetic; kernel may size lanes per model
    // per target: its job, trials per round, Love trials inside a lane group, and the trials of the group kernel's plan
    // (BH_DEBUG_PLAN prints these; the trial-per-lane kernel's differ)
    int job[BH_MAX_TARGETS], look[BH_MAX_TARGETS], inlook[BH_MAX_TARGETS], look_group[BH_MAX_TARGETS];
    // per target: takes the short refinement; a phase velocity that keeps the reference's sequence in a launch with it
    bool fast[BH_MAX_TARGETS], refseq[BH_MAX_TARGETS];
};

int swd_supported(bh_engine *e, int K, int iwave, int &igr, int mode, int flsph);
int wait_for(bh_engine *e, hipEvent_t ev, hipStream_t from, hipStream_t to);
SwdPlan plan_swd_call(const bh_engine *e, const ModelBatch &m, int njobs, const SwdJob *jobs);
int launch_swd_jobs(bh_engine *e, hipStream_t st, const ModelBatch &m, int njobs, const SwdJob *jobs, const SwdPlan &p,
                    const SwdFills &fills, int prio_low, SwdLaunchInfo *main);

// ---- the receiver function's argument rules (engine_eval.hip): bh_rf_batch's and a registered target's ----
int rf_args_ok(bh_engine *e, int nsamp, int nkeep, double gauss, double fsamp, int waveno);

} // namespace bheng

#endif
