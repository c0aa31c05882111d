// bayhunter_amd/csrc/bh_engine.hip -- host side of the C ABI declared in include/bh_engine.h.
//
// Owns the device workspace, the stream and the registered target data of one GPU, stages
// host buffers when the caller asks for memspace = BH_HOST and launches the gfx950 kernels of
// swd_kernel.hip / rf_kernel.hip / like_kernel.hip.  There is no CPU code path in here: if no
// HIP device is usable, bh_engine_create fails.
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
#include "bh_device.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "bh_tuning.h"
#include <cstring>
#include <mutex>

// ---- the experiment switches (bh_tuning.h) ----
namespace {
BhTuning g_tuning;
std::once_flag g_tuning_once;
int tuning_value(const char *env, const char *txt, int dflt)
{
    if (!txt) return dflt;
    if (!std::strcmp(env, "BH_SWD_SEARCH")) return (txt[0] == 'f' || txt[0] == '1') ? ((std::strstr(txt, "ray") || txt[0] == '2') ? BH_SEARCH_FAST_RAYLEIGH : BH_SEARCH_FAST) : (txt[0] == '2' ? BH_SEARCH_FAST_RAYLEIGH : BH_SEARCH_REFERENCE);
    if (!std::strcmp(env, "BH_SWD_ARITH")) return (txt[0] == 'e' || txt[0] == '0') ? BH_ARITH_EXACT : BH_ARITH_FAST;
    if (!std::strcmp(env, "BH_SWD_SCAN")) return (txt[0] == 's' || txt[0] == '0') ? BH_SCAN_STEPS : ((txt[0] == 'c' || txt[0] == '1') ? BH_SCAN_COUNTED : BH_SCAN_AUTO);
    char *end = nullptr;
    const long v = std::strtol(txt, &end, 10);
    if (end == txt) return 1; // a flag set to some text
    return (int)v;
}
// bounds: a switch can cost time, never memory safety (after the environment is parsed and after every bh_tuning_set)
void tuning_clamp()
{
    if (g_tuning.rf_lds_gated < 0 || g_tuning.rf_lds_gated > 160 * 1024) g_tuning.rf_lds_gated = 0;
    if (g_tuning.rf_lds_beside > 160 * 1024) g_tuning.rf_lds_beside = -1;
    if (g_tuning.swd_love_inlook < 0 || g_tuning.swd_love_inlook > 4) g_tuning.swd_love_inlook = 0;
    if (g_tuning.swd_gsplit < 0 || g_tuning.swd_gsplit > (1 << 24)) g_tuning.swd_gsplit = 0; // (the launch's entry index is an int)
}
void tuning_parse()
{
#ifndef BH_NO_EXPERIMENTS
#define X(field, env, dflt, doc) g_tuning.field = tuning_value(env, std::getenv(env), dflt);
    BH_TUNING_TABLE(X)
#undef X
    tuning_clamp();
#endif
    g_tuning.under_pmc = std::getenv("ROCPROF_COUNTER_COLLECTION") != nullptr ? 1 : 0;
}
} // namespace
const BhTuning &bh_tuning()
{
    std::call_once(g_tuning_once, tuning_parse);
    return g_tuning;
}
int bh_tuning_set(const char *name, int value)
{
#ifdef BH_NO_EXPERIMENTS
    (void)name; (void)value;
    return -1;
#else
    (void)bh_tuning();
    if (!name) return -1;
#define X(field, env, dflt, doc) if (!std::strcmp(name, #field)) { g_tuning.field = value; tuning_clamp(); return 0; }
    BH_TUNING_TABLE(X)
#undef X
    return -1;
#endif
}
int bh_tuning_get(const char *name, int *value)
{
    const BhTuning &t = bh_tuning();
    if (!name || !value) return -1;
#define X(field, env, dflt, doc) if (!std::strcmp(name, #field)) { *value = t.field; return 0; }
    BH_TUNING_TABLE(X)
#undef X
    return -1;
}

namespace {

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
};

void release(DevBuf &b)
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

} // namespace

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
    DevBuf nlay, h, vp, vs, rho, qp, qs, periods, vel, errb, rf, coef, ymod, noise, logL,
        misfits, err_t, probe_in, probe_out, counter, sph, perm, board, nevhi, rfz, gfirst, nevhi2;
    unsigned swd_stamp = 0;                // launch counter of the group kernel (marks its progress-board entries)
    // targets
    int nt = 0;
    int ldy = 0;
    std::vector<TargetHost> targets;
    SiteTable sites;                       // what the bh_sites_set* entry points registered for them
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
    DevBuf guard;        // short refinement: per target a count and a list of the models its guard fired on (re-run, see launch_swd_rerun)
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

// ---- the site part of a fused call's plan (bh_device.h): pure, no HIP call, no engine (tests/test_site_plan.py) ----
static_assert(BH_MAX_TARGETS == 8, "SitePlanAsk::t, SitePlan::gauss");
namespace {
const struct { int code; const char *text; } SITE_REFUSALS[] = { // by SiteRefusal
    {BH_OK, ""},
    {BH_EINVAL, "a BH_TARGET_USER target has no forward model: use bh_loglike_batch"},
    {BH_EINVAL, "bh_sites_set_missing with a receiver-function target needs bh_sites_set_rf"},
    {BH_EINVAL, "bh_sites_set_axes with a receiver-function count that differs from its descriptor's needs the table of bh_sites_set_rf_axis"},
    {BH_EINVAL, "bh_sites_set_missing_gauss with a Gauss-law target that a site lacks needs the table of bh_sites_set_gauss"},
    {BH_EINVAL, "bh_sites_set_laws with a Gauss-law target that has a site under another law needs the table of bh_sites_set_gauss (that site in class -1)"},
    {BH_EINVAL, "bh_sites_set_axes with a Gauss-law receiver function whose counts differ from its descriptor's needs the table of bh_sites_set_gauss (every site's matrix padded to the capacity)"},
    {BH_EUNSUPPORTED, "BH_NO_MFMA: the in-kernel mat-vec does not serve a Gauss-law receiver function with per-site counts (bh_sites_set_axes)"},
};
} // namespace
const char *bh_site_refusal_text(int refusal)
{
    return (refusal >= 0 && refusal <= REFUSE_RF_AXIS_NO_MFMA) ? SITE_REFUSALS[refusal].text : "";
}

SitePlan bh_plan_sites(const SitePlanAsk &q)
{
    SitePlan p{};
    bool have_rf = false, no_forward = false;
    for (int t = 0; t < q.nt; ++t) {
        have_rf = have_rf || q.t[t].kind == BH_TARGET_RF;
        no_forward = no_forward || (q.t[t].kind != BH_TARGET_SWD && q.t[t].kind != BH_TARGET_RF && q.t[t].kind != BH_TARGET_ELLIP);
    }
    // (periods per site: every dispersion job reads its models' periods and counts from the table)
    p.x_table = q.sites && q.level >= SITES_X;
    p.x_all = p.x_table && q.level >= SITES_X_ALL;
    // (sites with their own p / nsv: the coefficient kernels read them from the table, column t)
    p.rf_table = q.sites && q.rf;
    // (sites that lack targets: the coefficient stage looks the model's site up in the count table)
    p.missing = p.x_table && q.level >= SITES_MISSING;
    // (sites with their own time axis and filter: the synthesis kernel reads its model's site's record)
    p.rf_axis = p.rf_table && p.x_table && q.rf_axis;
    // (sites with their own noise law: the likelihood build that reads the law of (site, target) serves the call, with or without
    // class tables; the rows of a site under another law on a Gauss-law target must be in no tile of the contraction)
    p.laws = p.x_table && q.laws;
    p.like = p.missing ? LIKE_SITES_M : (p.x_table ? LIKE_SITES_X : (q.sites ? LIKE_SITES : LIKE_PLAIN));
    // (sites with their own noise correlation: a target with a class table is contracted class by class, and the likelihood build
    // that reads ln|R| of the model's class serves the call)
    bool own_no_axis = false, lacked_gauss = false, other_law_gauss = false, own_gauss = false, own_no_mfma = false;
    for (int t = 0; t < q.nt; ++t) {
        const SitePlanAsk::Target &T = q.t[t];
        const bool own = q.sites && T.rf_own_counts;
        p.gauss[t] = !q.sites ? GAUSS_PLAIN : (T.classes ? GAUSS_CLASSES : GAUSS_SITES);
        own_no_axis = own_no_axis || (own && !p.rf_axis);
        if (T.law != BH_LAW_GAUSS) continue;
        if (p.gauss[t] == GAUSS_CLASSES) p.like = LIKE_SITES_C;
        else if (q.sites && q.level >= SITES_MISSING_GAUSS && T.lacks) lacked_gauss = true;
        else if (own) own_gauss = true; // (the descriptor's matrix is the capacity's, no site's)
        // (the mat-vec's row stride is the site's n, the class matrices -- a site's in the corner of a zero matrix -- have the capacity's)
        own_no_mfma = own_no_mfma || (own && q.no_mfma);
        other_law_gauss = other_law_gauss || (p.laws && T.law_other && p.gauss[t] != GAUSS_CLASSES);
    }
    if (p.laws) p.like = LIKE_SITES_L;
    p.desc_counts = p.like == LIKE_SITES_C && !p.x_table;
    p.refusal = no_forward                               ? REFUSE_NO_FORWARD
                : (p.missing && have_rf && !p.rf_table) ? REFUSE_RF_NEEDS_TABLE
                : own_no_axis                            ? REFUSE_RF_AXIS_NEEDS_TABLE
                : lacked_gauss                           ? REFUSE_GAUSS_NEEDS_TABLE
                : other_law_gauss                        ? REFUSE_LAW_GAUSS_NEEDS_TABLE
                : own_gauss                              ? REFUSE_RF_AXIS_GAUSS_NEEDS_TABLE
                : own_no_mfma                            ? REFUSE_RF_AXIS_NO_MFMA
                                                         : REFUSE_NONE;
    p.code = SITE_REFUSALS[p.refusal].code;
    return p;
}

// ---- the ellipticity targets' part of a fused call's plan (include/bh_engine_ellip_target.h): pure, no HIP call, no engine ----
extern "C" int bh_plan_ellip(int nt, const bh_ellip_plan_target *T, int x_table, int32_t *source)
{
    if (nt < 0 || nt > BH_MAX_TARGETS || (nt > 0 && (!T || !source))) return -1;
    int own = 0;
    for (int t = 0; t < nt; ++t) {
        source[t] = -2;
        if (T[t].kind != BH_TARGET_ELLIP) continue;
        source[t] = -1;
        for (int j = 0; j < nt && !x_table && source[t] < 0; ++j) // (under a period table target j runs at its sites' periods)
            if (T[j].kind == BH_TARGET_SWD && T[j].iwave == BH_WAVE_RAYLEIGH && T[j].igr == BH_VEL_PHASE && T[j].mode <= 1 &&
                T[j].flsph == 0 && T[j].n <= BH_MAX_PERIODS && T[j].n == T[t].n && T[j].xid >= 0 && T[j].xid == T[t].xid)
                source[t] = j;
        own += source[t] < 0;
    }
    return own;
}

namespace {

int fail(bh_engine *e, int code, const char *what, hipError_t he = hipSuccess)
{
    if (e) {
        e->err = what;
        if (he != hipSuccess) {
            e->err += ": ";
            e->err += hipGetErrorString(he);
        }
    }
    return code;
}

#define HIPCHK(e, call)                                                  \
    do {                                                                 \
        hipError_t _he = (call);                                         \
        if (_he != hipSuccess) return fail((e), BH_EHIP, #call, _he);    \
    } while (0)

int ensure(bh_engine *e, DevBuf &b, size_t bytes)
{
    if (bytes <= b.cap) return BH_OK;
    if (b.p) {
        HIPCHK(e, hipStreamSynchronize(e->stream));
        if (e->aux) HIPCHK(e, hipStreamSynchronize(e->aux));
        if (e->aux2) HIPCHK(e, hipStreamSynchronize(e->aux2));
        HIPCHK(e, hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    size_t want = bytes + bytes / 4 + 256;
    hipError_t he = hipMalloc(&b.p, want);
    if (he != hipSuccess) return fail(e, BH_ENOMEM, "hipMalloc", he);
    b.cap = want;
    return BH_OK;
}

// every device buffer a registered target owns
void release_target(TargetHost &t)
{
    for (DevBuf *b : {&t.x, &t.yobs, &t.yerr_scaled, &t.rinv, &t.quad, &t.sums, &t.x60, &t.vel60, &t.ell_vel}) release(*b);
}

// Targets.py:124-128, the nocorr_scalederr law: out = yerr / min(yerr), returns ln prod(out) (bh_targets_set, bh_sites_set)
double scaled_errors(const double *yerr, int n, double *out)
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

// number of elements spanned by a strided [Lmax][B] view (strides must be positive)
size_t span_elems(int B, int Lmax, ptrdiff_t sl, ptrdiff_t sb)
{
    return (size_t)((ptrdiff_t)(Lmax - 1) * sl + (ptrdiff_t)(B - 1) * sb + 1);
}

__global__ void rho_from_vp_kernel(size_t n, const double *vp, double *rho)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) rho[i] = vp[i] * 0.32 + 0.77; // Targets.py:319
}

int check_models(bh_engine *e, int B, int Lmax, ptrdiff_t sl, ptrdiff_t sb)
{
    if (!e) return BH_EINVAL;
    if (B < 0 || Lmax < 1 || Lmax > BH_MAX_LAYERS) return fail(e, BH_EINVAL, "bad B or Lmax (1..100)");
    if (sl <= 0 || sb <= 0) return fail(e, BH_EINVAL, "strides must be positive");
    return BH_OK;
}

struct Staged {
    const int32_t *nlay;
    const double *h, *vp, *vs, *rho, *qp, *qs;
    int typ_layers = 0; // typical layer count of the batch when the host can see it (0 = unknown)
};

// Copy the model arrays of a BH_HOST call into the engine's device buffers: m's host pointers become device pointers
// (rho, qp and qs may be null and stay so).
int stage_models(bh_engine *e, int B, int Lmax, ptrdiff_t sl, ptrdiff_t sb, Staged &m)
{
    const size_t bytes = span_elems(B, Lmax, sl, sb) * sizeof(double);
    {   // mean layer count, rounded up: what the lanes-per-model choice should be sized for
        long sum = 0;
        for (int b = 0; b < B; ++b) sum += m.nlay[b];
        m.typ_layers = B > 0 ? (int)((sum + B - 1) / B) : 0;
    }
    int rc;
    if ((rc = ensure(e, e->nlay, (size_t)B * sizeof(int32_t)))) return rc;
    HIPCHK(e, hipMemcpyAsync(e->nlay.p, m.nlay, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    m.nlay = (const int32_t *)e->nlay.p;
    const double **arr[6] = {&m.h, &m.vp, &m.vs, &m.rho, &m.qp, &m.qs};
    DevBuf *buf[6] = {&e->h, &e->vp, &e->vs, &e->rho, &e->qp, &e->qs};
    for (int k = 0; k < 6; ++k) {
        if (!*arr[k]) continue;
        if ((rc = ensure(e, *buf[k], bytes))) return rc;
        HIPCHK(e, hipMemcpyAsync(buf[k]->p, *arr[k], bytes, hipMemcpyHostToDevice, e->stream));
        *arr[k] = (const double *)buf[k]->p;
    }
    return BH_OK;
}

bh_engine::EventSet *cur_set(bh_engine *e)
{
    return (e->timing && e->ncalls > 0) ? &e->evsets[e->ncalls - 1] : nullptr;
}
void ev_begin(bh_engine *e, int fam, hipStream_t st)
{
    bh_engine::EventSet *s = cur_set(e);
    if (!s) return;
    if (!s->used[fam]) { // first launch of this family in the call
        (void)hipEventRecord(s->ev[2 * fam], st);
        s->used[fam] = true;
    }
}
void ev_end(bh_engine *e, int fam, hipStream_t st)
{
    bh_engine::EventSet *s = cur_set(e);
    if (s) (void)hipEventRecord(s->ev[2 * fam + 1], st);
}
void call_begin(bh_engine *e, hipStream_t st)
{
    e->neval_pending = false;
    if (!e->timing) return;
    if (e->ncalls == e->evsets.size()) {
        bh_engine::EventSet s{};
        for (auto &ev : s.ev)
            if (hipEventCreate(&ev) != hipSuccess) return; // timing silently unavailable
        e->evsets.push_back(s);
    }
    bh_engine::EventSet &s = e->evsets[e->ncalls++];
    for (bool &u : s.used) u = false;
    (void)hipEventRecord(s.ev[6], st);
    s.used[3] = true;
}
void call_end(bh_engine *e, hipStream_t st)
{
    bh_engine::EventSet *s = cur_set(e);
    if (s) (void)hipEventRecord(s->ev[7], st);
}

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
constexpr int GUARD_HEAD = 24;
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

// What a target does in a fused call: nothing (a BH_TARGET_USER target has no forward model), dispersion at its own periods,
// dispersion on the 60-period grid followed by interpolation, a receiver function, or the ellipticity from the velocities of a
// dispersion target of the call or of a search of its own (include/bh_engine_ellip_target.h).
enum EvalRole { ROLE_NONE, ROLE_SWD, ROLE_SWD60, ROLE_RF, ROLE_ELLIP };
// What one fused call (bh_evaluate_batch, bh_evaluate_sites) does: everything its steps would otherwise decide.
struct EvalPlan {
    int B, nt, ldy;
    EvalRole role[BH_MAX_TARGETS];
    bool rf_fused[BH_MAX_TARGETS]; // receiver function: the synthesis kernel writes the likelihood's sums, not the trace
    int nswd;                   // dispersion jobs of the call: the dispersion targets' and the ellipticity targets' own searches
    int ell_source[BH_MAX_TARGETS]; // ROLE_ELLIP: the target whose velocities and failure flags it reads, or -1: a search of its own (bh_plan_ellip)
    bool fork;                  // the receiver functions run on the second stream, beside the dispersion launch
    bool want_gate;             // ... which waits for that launch's started workgroups (where the launch has any: gate_need)
    int prio_low;               // SwdMultiArgs::prio_low of the dispersion launch
    SitePlan sites;             // the site table's part (bh_plan_sites): the tables the launches read, the likelihood launcher, the refusal
    bool err_zero_always;       // bh_tuning.h err_memset: the failure flags are zeroed on every call
};

// What bh_plan_sites is asked about a fused call of engine e (sites: bh_evaluate_sites)
SitePlanAsk site_plan_ask(const bh_engine *e, bool sites)
{
    const SiteTable &S = e->sites;
    SitePlanAsk q{};
    q.sites = sites; q.level = S.level; q.rf = S.rf; q.rf_axis = S.rf_axis; q.laws = S.laws; q.no_mfma = e->no_mfma; q.nt = e->nt;
    for (int t = 0; t < q.nt; ++t) {
        const bh_target_desc &d = e->targets[(size_t)t].d;
        q.t[t] = SitePlanAsk::Target{d.kind, d.law, S.t[t].lacks, S.t[t].rf_own_counts, S.t[t].law_other, S.t[t].nclass > 0};
    }
    return q;
}

// The plan of one fused call, from the registered targets, the engine's settings, the experiment switches (bh_tuning.h) and the
// site table (its part: bh_plan_sites): no HIP call, no allocation, no write to the engine.  sites: bh_evaluate_sites; want_ymod: the caller asked
// for the synthetics.
EvalPlan plan_eval(const bh_engine *e, int B, bool sites, bool want_ymod)
{
    const BhTuning &tun = bh_tuning();
    EvalPlan p{};
    p.B = B; p.nt = e->nt; p.ldy = e->ldy;
    bool have_rf = false;
    for (int t = 0; t < p.nt; ++t) {
        const TargetHost &T = e->targets[(size_t)t];
        const bh_target_desc &d = T.d;
        if (d.kind == BH_TARGET_SWD) {
            p.role[t] = T.kfwd == d.n ? ROLE_SWD : ROLE_SWD60; // > 60 periods: run on the 60-point grid, interpolate afterwards
            ++p.nswd;
        } else if (d.kind == BH_TARGET_RF) {
            p.role[t] = ROLE_RF;
            have_rf = true;
            // Fused likelihood ("write nothing if the likelihood is fused"): the caller did not ask for the
            // synthetics and the target's law needs only sums over the trace -- the synthesis kernel forms them from the samples
            // in LDS (like_kernel's order: the same bits) and writes four numbers per model instead of the trace.
            // (sites: the trace goes to the ymod workspace and the site-indexed likelihood kernel forms the sums)
            p.rf_fused[t] = !want_ymod && !sites && tun.rf_no_fuse == 0 && (d.law == BH_LAW_NOCORR || d.law == BH_LAW_EXP) && tun.rf_threads != 128;
        }
    }
    // The receiver-function kernels are independent of the dispersion kernel and write other columns
    // of ymod: they run on a second stream so that their (throughput-bound) wavefronts fill the issue
    // slots the (latency-bound) dispersion wavefronts leave idle.  fork -> [swd | rf] -> join -> like.
    p.sites = bh_plan_sites(site_plan_ask(e, sites));
    {
        bh_ellip_plan_target q[BH_MAX_TARGETS];
        bool any = false;
        for (int t = 0; t < p.nt; ++t) {
            const TargetHost &T = e->targets[(size_t)t];
            q[t] = bh_ellip_plan_target{T.d.kind, T.d.iwave, T.d.igr, T.d.mode, T.d.flsph, T.d.n, T.xid};
            any = any || T.d.kind == BH_TARGET_ELLIP;
        }
        if (any) { // (the ids of SWD targets compare the DESCRIPTORS' periods: not what target j runs at under a period table)
            p.nswd += bh_plan_ellip(p.nt, q, p.sites.x_table, p.ell_source);
            for (int t = 0; t < p.nt; ++t)
                if (p.ell_source[t] != -2) p.role[t] = ROLE_ELLIP;
        }
    }
    p.fork = have_rf && p.nswd > 0 && e->overlap_rf;
    // Start gate.  The dispersion group kernel counts on ALL its wavefronts being co-resident (one round of wavefronts,
    // two per SIMD); an RF workgroup that takes a wave slot first displaces a dispersion wavefront for a whole lifetime
    // (3.6 -> 7 ms when the 17.7 KB workgroups of round 3 slipped into the LDS the dispersion wavefronts leave free), and
    // even the small coefficient kernel, dispatched while the dispersion kernel's workgroups are being placed, stretched
    // that kernel's span by 0.3 ms in round 2.  The kernel's workgroups therefore count themselves in `started` as they
    // begin, and the RF stream waits for the count (hipStreamWaitValue32) before anything of the RF is dispatched:
    // c3 4.15 -> 4.04 ms, the dispersion kernel's time inside c3 = its time in c2 (3.62 ms).
    // (Round 6: the dispersion kernel of the default settings allocates 200-208 registers and the synthesis kernel 88, so an RF
    // wavefront becomes resident beside the two dispersion wavefronts of a SIMD and takes the issue slots they leave idle; the
    // 96-register "beside" build of rounds 3-5 -- docs/HISTORY.md -- is gone.)
    p.want_gate = p.fork && e->started != nullptr;
    // (RF wavefronts move in beside the last dispersion wavefronts of a SIMD as its short ones end: the dispersion
    // wavefronts' unfavoured phase runs at priority 1 then, above the RF's 0)
    p.prio_low = p.want_gate ? e->swd_prio_low : 0;
    p.err_zero_always = tun.err_memset != 0;
    return p;
}

// The started workgroups of dispersion launch s the gated RF stream waits for: all workgroups of the launch, or -- a launch of
// more workgroups than the chip holds at once (2048 wavefronts) -- as many as can be resident together (the rest start as others
// end: waiting for them would be waiting for the kernel)
unsigned gate_need(const SwdLaunchInfo &s)
{
    const unsigned resident = 2048u / (unsigned)(s.lds > 0 && s.wpb > 0 ? s.wpb : 2);
    return s.workgroups < resident ? s.workgroups : resident;
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
    int B, Lmax; const Staged &m; ptrdiff_t sl, sb;
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
    t.h = c.m.h; t.vp = c.m.vp; t.vs = c.m.vs; t.rho = c.m.rho; t.sl = c.sl; t.sb = c.sb;
    if (J.flsph == 1) {
        const size_t ne = (size_t)c.Lmax * c.B;
        t.h = c.sph; t.vp = c.sph + ne; t.vs = c.sph + 2 * ne; t.rho = c.sph + (J.iwave == BH_WAVE_LOVE ? 3 : 4) * ne;
        t.sl = c.B; t.sb = 1;
    }
    t.periods = J.periods_dev; t.vel = J.vel; t.err = J.err;
    t.first = c.first[j];
    return t;
}

// the one-lane-per-model kernel's arguments of a target
SwdKernelArgs lane_args(const SwdCall &c, const SwdTarget &t)
{
    SwdKernelArgs a{};
    a.B = c.B; a.Lmax = c.Lmax; a.K = t.K; a.igr = t.igr; a.mode = t.mode; a.perm = c.perm;
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

// stream `to` waits for what `from` has enqueued so far: the fork to and the join from the engine's second stream, on which
// every second launch of a call runs side by side with the others
int wait_for(bh_engine *e, hipEvent_t ev, hipStream_t from, hipStream_t to)
{
    HIPCHK(e, hipEventRecord(ev, from));
    HIPCHK(e, hipStreamWaitEvent(to, ev, 0));
    return BH_OK;
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
    const int nt = c.p.ntargets, B = c.B;
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
    c.order_wgs = bh_launch_pair_order(B, c.Lmax, c.m.nlay, t0.vs, t0.sl, t0.sb, ok ? nt : 0, tg, c.fills, c.st);
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
    if ((rc = ensure(e, e->perm, ((size_t)c.B + 4) * sizeof(int32_t)))) return rc;
    int32_t *perm = (int32_t *)e->perm.p;
    if (p.order == ORDER_LENGTH) {
        const PairOrderTarget tg{p.len_mpw, c.B / p.len_mpw, nullptr, perm + 4, p.len_xcd};
        c.order_wgs = bh_launch_pair_order(c.B, c.Lmax, c.m.nlay, c.m.vs, c.sl, c.sb, 1, &tg, c.fills, c.st);
    } else {
        bh_launch_order(c.B, c.m.nlay, perm + 4, p.Lcut, perm, c.st);
        c.order_wgs = 1;
        c.split = (p.Lcut < c.Lmax) ? perm : nullptr;
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
    const int B = c.B, n = p.ntargets;
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
    ra.B = B; ra.Lmax = c.Lmax; ra.nlay = c.m.nlay; ra.neval = c.counter; ra.counted = e->swd_scan;
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
    const int B = c.B;
    int rc;
    if ((rc = swd_board(e, c.st, &a.board))) return rc;
    a.stamp = swd_stamp(e);
    a.B = B; a.Lmax = c.Lmax; a.nlay = c.m.nlay; a.neval = c.counter; a.perm = c.perm;
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
                     B, c.Lmax, p.G, c.m.typ_layers, e->hint_layers, p.Lcut, p.Lcut < c.Lmax ? " (two depth classes)" : "", (int)(p.order == ORDER_PAIR));
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
    const int B = c.B;
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

// The plan of a call's dispersion jobs on the staged batch m (no dispersion job: a plan without targets, order or prologue)
SwdPlan plan_swd_call(const bh_engine *e, int B, int Lmax, const Staged &m, int njobs, const SwdJob *jobs)
{
    return plan_swd(e, B, Lmax, m.typ_layers > 0 ? m.typ_layers : e->hint_layers, njobs, jobs);
}

// All dispersion targets of one call: the plan, the flattened copies and the order it needs, then its launches -- the group or
// trial-per-lane kernel (one launch for all targets) or one lane per model (a launch per target) -- the re-run of the models
// the guard of the short refinement fired on, and the second roots of split group velocities.
// p: the call's plan (plan_swd_call).  fills: where p.prologue, what the caller leaves to the ordering launch to zero (the guard's
// head and the counters are added here).  prio_low: SwdMultiArgs::prio_low of the main launch.  main: null, or where the
// SwdLaunchInfo of the call's main launch goes once the call has dispersion targets (workgroups == 0: not a launch of the group
// or trial-per-lane kernel).
int launch_swd_jobs(bh_engine *e, hipStream_t st, int B, int Lmax, const Staged &m, ptrdiff_t sl, ptrdiff_t sb, int njobs,
                    const SwdJob *jobs, const SwdPlan &p, const SwdFills &fills, int prio_low, SwdLaunchInfo *main)
{
    if (B == 0 || njobs == 0) return BH_OK;
    SwdCall c{e, st, B, Lmax, m, sl, sb, jobs, p};
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
        bh_launch_sphere(B, Lmax, m.nlay, m.h, m.vp, m.vs, m.rho, sl, sb, base, base + ne, base + 2 * ne, base + 3 * ne, base + 4 * ne, st);
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

// What one receiver-function launch synthesises: the descriptor's numbers, the output rows, the inputs of the fused
// likelihood (yobs and sums, or null: the trace is written), the build and the site table it reads (RF_PLAIN: none).
struct RfJob {
    double p, gauss;
    int nsamp;
    double fsamp, tshift, nsv;
    int waveno, nkeep;
    double *rf; int ldr;
    const double *yobs; double *sums;
    RfBuild build;
    RfSiteTArgs sites; // (a build reads the base it needs)
};

// The build of a fused call's receiver-function launches, by the tables its site plan has in force
RfBuild rf_build(const SitePlan &sp)
{
    return sp.rf_axis ? RF_SITEAXIS : sp.missing ? RF_MISSING : sp.rf_table ? RF_SITES : RF_PLAIN;
}

// Ask, plan (bh_plan_rf, rf_plan.hip: every rule is there), launch.  beside_swd, gated: where the launch sits (RfAsk)
int launch_rf(bh_engine *e, hipStream_t st, int B, int Lmax, const Staged &m, ptrdiff_t sl, ptrdiff_t sb, const RfJob &j, bool beside_swd, bool gated)
{
    if (B == 0) return BH_OK;
    const RfAsk q{B, Lmax, j.build, j.build == RF_SITEAXIS ? j.sites.nsamp_max : j.nsamp, j.fsamp, j.gauss, beside_swd, gated, e->rf_lds_beside_swd};
    const RfPlan p = bh_plan_rf(q, bh_tuning());
    if (p.code != BH_OK) return fail(e, p.code, bh_rf_refusal_text(p.refusal));
    if (int rc = ensure(e, e->coef, (size_t)B * bh_rf_coef_doubles(Lmax) * sizeof(double))) return rc;
    if (int rc = p.workspace ? ensure(e, e->rfz, p.work_bytes) : BH_OK) return rc;
    RfKernelArgs a{}; // (lds_min and coef_small stay 0: unused)
    a.B = B; a.Lmax = Lmax; a.nsamp = j.nsamp; a.nkeep = j.nkeep; a.waveno = j.waveno;
    a.nlay = m.nlay; a.h = m.h; a.vp = m.vp; a.vs = m.vs; a.rho = m.rho; a.qp = m.qp; a.qs = m.qs; a.sl = sl; a.sb = sb;
    a.p_s_per_deg = j.p; a.gauss = j.gauss; a.fsamp = j.fsamp; a.tshift = j.tshift; a.nsv = j.nsv;
    a.coef = (double *)e->coef.p; a.rf = j.rf; a.ldr = j.ldr;
    a.yobs = j.yobs; a.sums = j.sums; // (fused likelihood: the sums instead of the trace)
    a.zwork = p.workspace ? (double *)e->rfz.p : nullptr;
    a.no_realc = p.no_realc; a.no_rot = p.no_rot;
    int (*const launcher[RF_BUILDS])(const RfPlan &, const RfKernelArgs &, const RfSiteTArgs *, hipStream_t) = {bh_launch_rf, bh_launch_rf, bh_launch_rf_m, bh_launch_rf_t};
    ev_begin(e, 1, st);
    const int lrc = launcher[j.build](p, a, j.build == RF_PLAIN ? nullptr : &j.sites, st);
    ev_end(e, 1, st);
    if (lrc != BH_OK) return fail(e, lrc, lrc == BH_EHIP ? bh_rf_refusal_text(RF_REFUSE_ALLOWANCE) : "receiver function: a plan its build does not serve");
    HIPCHK(e, hipGetLastError());
    return BH_OK;
}

// Fill the likelihood descriptor L of target t; for the Gauss law run the MFMA contraction first.
// site: null, or the site index of every model (device; bh_evaluate_sites): the Gauss contraction reads the observed data
// of each model's site from the site table.  fused: the target's likelihood comes from the sums of this call's synthesis launch
// (EvalPlan::rf_fused), not from ymod
int prepare_like_target(bh_engine *e, hipStream_t st, int B, int ldy, const double *ymod_d, int t,
                        LikeTargetDev &L, bool fused, const int32_t *site, EvalGauss how)
{
    TargetHost &T = e->targets[(size_t)t];
    SiteTable &S = e->sites;
    L.law = T.d.law; L.n = T.d.n; L.off = T.off;
    L.yobs = (const double *)T.yobs.p;
    L.yerr_scaled = (const double *)T.yerr_scaled.p;
    L.rinv = (const double *)T.rinv.p;
    L.logdet_extra = T.logdet_extra;
    L.quad = nullptr;
    L.nsplit = 0;
    L.pre = fused ? (const double *)T.sums.p : nullptr;
    if (T.d.law == BH_LAW_GAUSS && !e->no_mfma) {
        const int nsplit = bh_gauss_nsplit(B, T.d.n);
        int rc = ensure(e, T.quad, (size_t)B * nsplit * sizeof(double));
        if (rc) return rc;
        if (how == GAUSS_CLASSES && (rc = ensure(e, S.class_work, bh_gauss_class_work_words(B, S.t[t].nclass) * sizeof(int32_t)))) return rc;
        ev_begin(e, 2, st);
        if (how == GAUSS_CLASSES) { // (grouping launches + the contraction over tiles of one class each)
            const GaussSiteArgs gs{site, S.nsites, ldy};
            bh_launch_gauss_quad_classes(B, T.d.n, ldy, ymod_d + T.off, (const double *)S.yobs.p + T.off, gs, (const int32_t *)S.t[t].class_of.p,
                                         S.t[t].nclass, (const double *)S.t[t].rinv.p, nsplit, (double *)T.quad.p, (int32_t *)S.class_work.p, st);
        } else if (site) {
            const GaussSiteArgs gs{site, S.nsites, ldy};
            bh_launch_gauss_quad_sites(B, T.d.n, ldy, ymod_d + T.off, (const double *)S.yobs.p + T.off, gs, L.rinv, nsplit,
                                       (double *)T.quad.p, st);
        } else {
            bh_launch_gauss_quad(B, T.d.n, ldy, ymod_d + T.off, L.yobs, L.rinv, nsplit, (double *)T.quad.p, st);
        }
        L.quad = (const double *)T.quad.p;
        L.nsplit = nsplit;
    }
    return BH_OK;
}

int rf_args_ok(bh_engine *e, int nsamp, int nkeep, double gauss, double fsamp, int waveno)
{
    if (nsamp < 4 || (nsamp & (nsamp - 1)) != 0)
        return fail(e, BH_EINVAL, "nsamp must be a power of two >= 4");
    // rfmini_modrf.py:62 derives nsamp = 2^ceil(log2(2 ndata)) with no upper bound; here one workgroup holds a model's
    // half-length complex spectrum in LDS up to 16384 samples and in an HBM workspace beyond, up to 2^18 samples
    if (nsamp > BH_RF_MAX_NSAMP)
        return fail(e, BH_EUNSUPPORTED, "nsamp above 262144 is not supported");
    if (nkeep < 0 || nkeep > nsamp) return fail(e, BH_EINVAL, "nkeep must be 0..nsamp");
    if (!(gauss > 0.0) || !(fsamp > 0.0)) return fail(e, BH_EINVAL, "gauss and fsamp must be > 0");
    if (waveno != BH_RF_P && waveno != BH_RF_SV) return fail(e, BH_EINVAL, "waveno must be 0 (P) or 1 (SV)");
    return BH_OK;
}

} // namespace

extern "C" {

int bh_abi_version(void) { return BH_ABI_VERSION; }

int bh_engine_create(int device, bh_engine **out)
{
    if (!out) return BH_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return BH_EHIP;
    if (device < 0 || device >= ndev) return BH_EINVAL;
    bh_engine *e = new (std::nothrow) bh_engine;
    if (!e) return BH_ENOMEM;
    e->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&e->stream) != hipSuccess ||
        hipStreamCreateWithFlags(&e->aux, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipStreamCreateWithFlags(&e->aux2, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_fork2, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_join2, hipEventDisableTiming) != hipSuccess) {
        delete e;
        return BH_EHIP;
    }
    const BhTuning &tun = bh_tuning(); // (the experiment switches: parsed once per process, bh_tuning.h)
    if (tun.no_overlap) e->overlap_rf = false;
    if (tun.rf_lds_beside >= 0) e->rf_lds_beside_swd = tun.rf_lds_beside;
    {
        hipDeviceProp_t prop;
        e->pairwork.ncu = (hipGetDeviceProperties(&prop, device) == hipSuccess) ? prop.multiProcessorCount : 0;
    }
    if (tun.swd_prio_low >= 0) e->swd_prio_low = tun.swd_prio_low != 0 ? 1 : 0;
    {   // the counter the dispersion kernel's workgroups bump at start; hipStreamWaitValue32 polls it from the RF stream
        int can = 0;
        (void)hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, device);
        if (tun.no_started) can = 0;
        // rocprofv3 --pmc (counter collection) runs the dispatches of ALL queues one at a time; the RF stream's wait
        // packet then never sees the dispersion kernel start (measured: bench.py --workload c3 hangs under --pmc, runs
        // under --kernel-trace).  The gate is a scheduling aid only: off in that mode.
        if (tun.under_pmc) can = 0;
        // plain device memory: the wait packet polls it just as well, and atomics on signal memory
        // (hipMallocSignalMemory) cost the dispersion kernel 1 ms per launch (976 workgroups, one atomic each)
        if (can && hipMalloc((void **)&e->started, 8) != hipSuccess) e->started = nullptr;
        if (e->started && hipMemset(e->started, 0, 8) != hipSuccess) {
            (void)hipFree(e->started);
            e->started = nullptr;
        }
        (void)hipGetLastError();
    }
    e->force_group = tun.swd_group;
    e->force_look = tun.swd_lookahead;
    if (tun.swd_search >= 0) e->swd_search = tun.swd_search;
    if (tun.swd_arith >= 0) e->swd_arith = tun.swd_arith != 0 ? BH_ARITH_FAST : BH_ARITH_EXACT;
    if (tun.swd_scan >= 0) e->swd_scan = tun.swd_scan;
    if (tun.no_mfma) e->no_mfma = true;
    *out = e;
    return BH_OK;
}

int bh_engine_set_typical_layers(bh_engine *e, int nlay)
{
    if (!e) return BH_EINVAL;
    if (nlay < 0 || nlay > BH_MAX_LAYERS) return fail(e, BH_EINVAL, "typical layer count must be 0 (unknown) or 1..100");
    e->hint_layers = nlay;
    return BH_OK;
}

int bh_engine_set_model_order(bh_engine *e, int sort_by_depth)
{
    if (!e) return BH_EINVAL;
    e->as_given = (sort_by_depth == 0);
    return BH_OK;
}

int bh_engine_set_swd_search(bh_engine *e, int search)
{
    if (!e) return BH_EINVAL;
    if (search != BH_SEARCH_REFERENCE && search != BH_SEARCH_FAST && search != BH_SEARCH_FAST_RAYLEIGH)
        return fail(e, BH_EINVAL, "search must be BH_SEARCH_REFERENCE (0), BH_SEARCH_FAST (1) or BH_SEARCH_FAST_RAYLEIGH (2)");
    e->swd_search = search;
    return BH_OK;
}

int bh_engine_get_swd_search(const bh_engine *e) { return e ? e->swd_search : 0; }

int bh_engine_set_swd_scan(bh_engine *e, int scan)
{
    if (!e) return BH_EINVAL;
    if (scan != BH_SCAN_STEPS && scan != BH_SCAN_COUNTED && scan != BH_SCAN_AUTO) return fail(e, BH_EINVAL, "scan must be BH_SCAN_STEPS, BH_SCAN_COUNTED or BH_SCAN_AUTO");
    e->swd_scan = scan;
    return BH_OK;
}
int bh_engine_get_swd_scan(const bh_engine *e) { return e ? e->swd_scan : 0; }

int bh_engine_set_tuning(bh_engine *e, const char *name, int value)
{
    if (!e) return BH_EINVAL;
    if (bh_tuning_set(name, value) != 0) return fail(e, BH_EINVAL, "unknown experiment switch (csrc/bh_tuning.h), or a build with BH_NO_EXPERIMENTS");
    return BH_OK;
}
int bh_engine_get_tuning(bh_engine *e, const char *name, int *value)
{
    if (!e) return BH_EINVAL;
    if (bh_tuning_get(name, value) != 0) return fail(e, BH_EINVAL, "unknown experiment switch (csrc/bh_tuning.h)");
    return BH_OK;
}

int bh_engine_set_swd_arith(bh_engine *e, int arith)
{
    if (!e) return BH_EINVAL;
    if (arith != BH_ARITH_EXACT && arith != BH_ARITH_FAST) return fail(e, BH_EINVAL, "arith must be BH_ARITH_EXACT (0) or BH_ARITH_FAST (1)");
    e->swd_arith = arith;
    return BH_OK;
}
int bh_engine_get_swd_arith(const bh_engine *e) { return e ? e->swd_arith : 0; }
int bh_engine_last_swd_kernel(const bh_engine *e) { return e ? e->last_swd_kernel : -1; }
int bh_engine_last_swd_perm(bh_engine *e, int target, int32_t *out, int n)
{
    if (!e || !out || target < 0 || target > 1 || n < 0) return BH_EINVAL;
    if (e->last_swd_perm[target] == nullptr) return 0;
    if (n < e->last_swd_perm_n) return BH_EINVAL;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemcpy(out, e->last_swd_perm[target], (size_t)e->last_swd_perm_n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return e->last_swd_perm_n;
}
int bh_engine_last_swd_order(const bh_engine *e, int *workgroups, int *fills)
{
    if (workgroups) *workgroups = e ? e->last_swd_order[1] : 0;
    if (fills) *fills = e ? e->last_swd_order[2] : 0;
    return e ? e->last_swd_order[0] : -1;
}
int bh_engine_last_swd_launches(const bh_engine *e, bh_swd_launch *out, int max, int *n)
{
    if (!e || !n || max < 0 || (max > 0 && !out)) return BH_EINVAL;
    const int m = e->n_swd_launches < max ? e->n_swd_launches : max;
    for (int i = 0; i < m; ++i) out[i] = e->swd_launches[i];
    *n = m;
    return BH_OK;
}
int bh_engine_set_swd_trials(bh_engine *e, int trials)
{
    if (!e) return BH_EINVAL;
    if (trials != 0 && trials != 4 && trials != 8 && trials != 16 && trials != 32 && trials != 64)
        return fail(e, BH_EINVAL, "trials must be 0 (by the call's shape), 4, 8, 16, 32 or 64");
    e->swd_trials = trials;
    return BH_OK;
}
int bh_engine_get_swd_trials(const bh_engine *e) { return e ? e->swd_trials : 0; }
int bh_engine_guard_stats(bh_engine *e, int32_t *counts, uint64_t *rerun_launches, uint64_t *total)
{
    if (!e) return BH_EINVAL;
    if (rerun_launches) *rerun_launches = e->rerun_launches;
    if (counts || total) {
        int32_t w[3 * BH_MAX_TARGETS] = {0};
        if (e->guard.p && !e->guard_fresh) {
            HIPCHK(e, hipDeviceSynchronize()); // (the last call may have run on a caller's stream)
            HIPCHK(e, hipMemcpy(w, e->guard.p, sizeof(w), hipMemcpyDeviceToHost));
        }
        if (counts)
            for (int t = 0; t < BH_MAX_TARGETS; ++t) counts[t] = e->guard_last ? w[t] + w[BH_MAX_TARGETS + t] : 0;
        if (total)
            for (int t = 0; t < BH_MAX_TARGETS; ++t) total[t] = e->guard_total[t] + (uint64_t)(uint32_t)w[2 * BH_MAX_TARGETS + t];
    }
    return BH_OK;
}

int bh_engine_set_swd_lookahead(bh_engine *e, int trials_per_round)
{
    if (!e) return BH_EINVAL;
    if (trials_per_round < 0 || trials_per_round > 16)
        return fail(e, BH_EINVAL, "look-ahead must be 0 (auto) or 1..16 trial velocities per round");
    e->force_look = trials_per_round;
    return BH_OK;
}

int bh_engine_set_swd_group(bh_engine *e, int lanes_per_model)
{
    if (!e) return BH_EINVAL;
    if (lanes_per_model < 0 || lanes_per_model > 32)
        return fail(e, BH_EINVAL, "lanes per model must be 0 (auto) or 1..32");
    e->force_group = lanes_per_model;
    return BH_OK;
}

void bh_engine_destroy(bh_engine *e)
{
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    for (DevBuf *b : {&e->nlay, &e->h, &e->vp, &e->vs, &e->rho, &e->qp, &e->qs, &e->periods, &e->vel,
                      &e->errb, &e->rf, &e->coef, &e->ymod, &e->noise, &e->logL, &e->misfits,
                      &e->err_t, &e->probe_in, &e->probe_out, &e->counter, &e->sph, &e->perm, &e->board, &e->nevhi, &e->guard, &e->rfz, &e->gfirst, &e->nevhi2})
        release(*b);
    for (auto &t : e->targets) release_target(t);
    e->sites.drop(PART_COUNTS);
    release(e->sites.class_work);
    for (auto &s : e->evsets)
        for (auto &ev : s.ev)
            if (ev) (void)hipEventDestroy(ev);
    if (e->started) (void)hipFree(e->started);
    for (int t = 0; t < 2; ++t) {
        if (e->pairwork.perm[t]) (void)hipFree(e->pairwork.perm[t]);
        if (e->pairwork.slot_rank[t]) (void)hipFree(e->pairwork.slot_rank[t]);
    }
    if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
    if (e->ev_join) (void)hipEventDestroy(e->ev_join);
    if (e->aux) (void)hipStreamDestroy(e->aux);
    if (e->ev_fork2) (void)hipEventDestroy(e->ev_fork2);
    if (e->ev_join2) (void)hipEventDestroy(e->ev_join2);
    if (e->aux2) (void)hipStreamDestroy(e->aux2);
    (void)hipStreamDestroy(e->stream);
    delete e;
}

const char *bh_engine_last_error(const bh_engine *e) { return e ? e->err.c_str() : "null engine"; }

} // extern "C"

int bh_engine_fail_internal(bh_engine *e, int code, const char *what) { return fail(e, code, what); }
int bh_engine_device_internal(const bh_engine *e) { return e->device; }

extern "C" {
void *bh_engine_stream(bh_engine *e) { return e ? (void *)e->stream : nullptr; }

int bh_engine_synchronize(bh_engine *e)
{
    if (!e) return BH_EINVAL;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return BH_OK;
}

int bh_engine_set_instrumentation(bh_engine *e, int timing, int counting)
{
    if (!e) return BH_EINVAL;
    e->timing = timing != 0;
    e->counting = counting != 0;
    return BH_OK;
}

int bh_timing_reset(bh_engine *e)
{
    if (!e) return BH_EINVAL;
    e->ncalls = 0;
    return BH_OK;
}

int bh_timing_collect(bh_engine *e, int *ncalls, double *total_ms, double family_ms[3])
{
    if (!e) return BH_EINVAL;
    double tot = 0.0, fam[3] = {0.0, 0.0, 0.0};
    for (size_t i = 0; i < e->ncalls; ++i) {
        bh_engine::EventSet &s = e->evsets[i];
        HIPCHK(e, hipEventSynchronize(s.ev[7]));
        float ms = 0.f;
        HIPCHK(e, hipEventElapsedTime(&ms, s.ev[6], s.ev[7]));
        tot += ms;
        for (int f = 0; f < 3; ++f) {
            if (!s.used[f]) continue;
            float fm = 0.f;
            HIPCHK(e, hipEventElapsedTime(&fm, s.ev[2 * f], s.ev[2 * f + 1]));
            fam[f] += fm;
        }
    }
    if (ncalls) *ncalls = (int)e->ncalls;
    if (total_ms) *total_ms = tot;
    if (family_ms)
        for (int f = 0; f < 3; ++f) family_ms[f] = fam[f];
    return BH_OK;
}

int bh_timing_steps(bh_engine *e, int max, double *step_ms, int *n)
{
    if (!e || !step_ms || !n || max < 0) return BH_EINVAL;
    int k = 0;
    for (size_t i = 0; i < e->ncalls && k < max; ++i, ++k) {
        bh_engine::EventSet &s = e->evsets[i];
        HIPCHK(e, hipEventSynchronize(s.ev[7]));
        float ms = 0.f;
        if (i + 1 < e->ncalls) HIPCHK(e, hipEventElapsedTime(&ms, s.ev[6], e->evsets[i + 1].ev[6]));
        else HIPCHK(e, hipEventElapsedTime(&ms, s.ev[6], s.ev[7]));
        step_ms[k] = ms;
    }
    *n = k;
    return BH_OK;
}

int bh_debug_counters(bh_engine *e, uint64_t out[16])
{
    if (!e || !out) return BH_EINVAL;
    if (!e->counter.p) return fail(e, BH_EINVAL, "counting was never enabled");
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemcpy(out, e->counter.p, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return BH_OK;
}

int bh_debug_trace(bh_engine *e, uint64_t *out, int nwaves)
{
    if (!e || !out || nwaves < 0 || nwaves > BH_TRACE_WAVES) return BH_EINVAL;
    if (!e->counter.p) return fail(e, BH_EINVAL, "counting was never enabled");
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemcpy(out, (uint64_t *)e->counter.p + BH_COUNTER_WORDS, (size_t)4 * nwaves * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return BH_OK;
}

int bh_debug_guard_list(bh_engine *e, int target, int B, int32_t *out, int max, int *n)
{
    if (!e || !n || target < 0 || target >= BH_MAX_TARGETS || B < 0 || max < 0 || (max > 0 && !out)) return BH_EINVAL;
    *n = 0;
    if (!e->guard.p || e->guard_fresh || !e->guard_last) return BH_OK;
    if (((size_t)GUARD_HEAD + (size_t)(target + 1) * (size_t)(B + 4)) * sizeof(int32_t) > e->guard.cap) return fail(e, BH_EINVAL, "not the last call's batch size");
    int32_t cnt = 0;
    HIPCHK(e, hipDeviceSynchronize()); // (the last call may have run on a caller's stream)
    HIPCHK(e, hipMemcpy(&cnt, (int32_t *)e->guard.p + target, sizeof(cnt), hipMemcpyDeviceToHost));
    if (cnt < 0 || cnt > B) return fail(e, BH_EINVAL, "not the last call's batch size");
    const int m = cnt < max ? cnt : max;
    if (m > 0) HIPCHK(e, hipMemcpy(out, (int32_t *)e->guard.p + GUARD_HEAD + (size_t)target * (size_t)(B + 4), (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));
    *n = m;
    return BH_OK;
}

int bh_last_neval(bh_engine *e, uint64_t *neval)
{
    if (!e || !neval) return BH_EINVAL;
    if (e->neval_pending) {
        unsigned long long v = 0;
        HIPCHK(e, hipMemcpy(&v, e->counter.p, sizeof(v), hipMemcpyDeviceToHost));
        e->last_neval = v;
        e->neval_pending = false;
    }
    *neval = e->last_neval;
    return BH_OK;
}

int bh_swd_batch(bh_engine *e, int memspace, void *stream, int B, int Lmax, const int32_t *nlay,
                 const double *h, const double *vp, const double *vs, const double *rho,
                 ptrdiff_t sl, ptrdiff_t sb, int K, const double *periods, int iwave, int igr,
                 int mode, int flsph, double *vel, int32_t *err)
{
    int rc;
    if ((rc = check_models(e, B, Lmax, sl, sb))) return rc;
    if ((rc = swd_supported(e, K, iwave, igr, mode, flsph))) return rc;
    if (!nlay || !h || !vp || !vs || !rho || !periods || !vel || !err) return fail(e, BH_EINVAL, "null argument");
    if (B == 0) return BH_OK;
    HIPCHK(e, hipSetDevice(e->device));
    const bool host = (memspace != BH_DEVICE);
    hipStream_t st = (!host && stream) ? (hipStream_t)stream : e->stream;
    Staged m{nlay, h, vp, vs, rho, nullptr, nullptr};
    SwdJob job{K, iwave, igr, K, periods, vel, err, mode, flsph};
    if (host) {
        if ((rc = stage_models(e, B, Lmax, sl, sb, m))) return rc;
        if ((rc = ensure(e, e->periods, (size_t)BH_MAX_PERIODS * sizeof(double)))) return rc;
        if ((rc = ensure(e, e->vel, (size_t)B * K * sizeof(double)))) return rc;
        if ((rc = ensure(e, e->errb, (size_t)B * sizeof(int32_t)))) return rc;
        HIPCHK(e, hipMemcpyAsync(e->periods.p, periods, (size_t)K * sizeof(double), hipMemcpyHostToDevice, st));
        job.periods_dev = (const double *)e->periods.p; job.vel = (double *)e->vel.p; job.err = (int32_t *)e->errb.p;
    }
    call_begin(e, st);
    rc = launch_swd_jobs(e, st, B, Lmax, m, sl, sb, 1, &job, plan_swd_call(e, B, Lmax, m, 1, &job), SwdFills{}, 0, nullptr);
    call_end(e, st);
    if (rc || !host) return rc;
    HIPCHK(e, hipMemcpyAsync(vel, e->vel.p, (size_t)B * K * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipMemcpyAsync(err, e->errb.p, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    return BH_OK;
}

int bh_rf_batch(bh_engine *e, int memspace, void *stream, int B, int Lmax, const int32_t *nlay,
                const double *h, const double *vp, const double *vs, const double *rho,
                const double *qp, const double *qs, ptrdiff_t sl, ptrdiff_t sb, double p,
                double gauss, int nsamp, double fsamp, double tshift, double nsv, int waveno,
                int nkeep, double *rf)
{
    int rc;
    if ((rc = check_models(e, B, Lmax, sl, sb))) return rc;
    if ((rc = rf_args_ok(e, nsamp, nkeep, gauss, fsamp, waveno))) return rc;
    if (!nlay || !h || !vp || !vs || !rho || !rf) return fail(e, BH_EINVAL, "null argument");
    if (B == 0 || nkeep == 0) return BH_OK;
    HIPCHK(e, hipSetDevice(e->device));
    const bool host = (memspace != BH_DEVICE);
    hipStream_t st = (!host && stream) ? (hipStream_t)stream : e->stream;
    Staged m{nlay, h, vp, vs, rho, qp, qs};
    RfJob job{p, gauss, nsamp, fsamp, tshift, nsv, waveno, nkeep, rf, nkeep, nullptr, nullptr, RF_PLAIN, RfSiteTArgs{}};
    if (host) {
        if ((rc = stage_models(e, B, Lmax, sl, sb, m))) return rc;
        if ((rc = ensure(e, e->rf, (size_t)B * nkeep * sizeof(double)))) return rc;
        job.rf = (double *)e->rf.p;
    }
    call_begin(e, st);
    rc = launch_rf(e, st, B, Lmax, m, sl, sb, job, false, false); // (not beside anything)
    call_end(e, st);
    if (rc || !host) return rc;
    HIPCHK(e, hipMemcpyAsync(rf, e->rf.p, (size_t)B * nkeep * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    return BH_OK;
}

// The id of the bit pattern of target i's periods (x_host) among targets 0 .. i-1 and itself: the id of the first with the same
// bits, else one more than the largest
static int period_id(const std::vector<TargetHost> &ts, int i, int upto = -1)
{
    const std::vector<double> &x = ts[(size_t)i].x_host;
    int next = 0;
    for (int j = 0; j < (upto < 0 ? i : upto); ++j) {
        if (j == i) continue;
        const TargetHost &o = ts[(size_t)j];
        if (o.xid < 0) continue;
        if (o.x_host.size() == x.size() && std::memcmp(o.x_host.data(), x.data(), x.size() * sizeof(double)) == 0) return o.xid;
        next = std::max(next, o.xid + 1);
    }
    return next;
}

int bh_targets_set(bh_engine *e, int nt, const bh_target_desc *td)
{
    if (!e) return BH_EINVAL;
    if (nt < 0 || nt > BH_MAX_TARGETS || (nt > 0 && !td)) return fail(e, BH_EINVAL, "nt must be 0..8");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    for (auto &t : e->targets) release_target(t);
    e->sites.drop(PART_COUNTS);
    e->targets.clear();
    e->nt = 0;
    e->ldy = 0;
    int off = 0;
    std::vector<TargetHost> tmp((size_t)nt);
    for (int i = 0; i < nt; ++i) {
        const bh_target_desc &d = td[i];
        TargetHost &t = tmp[(size_t)i];
        t.d = d;
        t.off = off;
        int rc = BH_OK;
        if (d.n < 1 || !d.yobs) rc = fail(e, BH_EINVAL, "target needs n >= 1 and yobs");
        if (!rc && d.law != BH_LAW_NOCORR && d.law != BH_LAW_NOCORR_SCALED && d.law != BH_LAW_EXP && d.law != BH_LAW_GAUSS)
            rc = fail(e, BH_EINVAL, "unknown covariance law");
        if (!rc && d.kind == BH_TARGET_SWD) {
            if (!d.x) rc = fail(e, BH_EINVAL, "SWD target needs periods x");
            if (!rc) rc = swd_supported(e, d.n > BH_MAX_PERIODS ? BH_MAX_PERIODS : d.n, d.iwave, t.d.igr, d.mode, d.flsph);
        } else if (!rc && d.kind == BH_TARGET_RF) {
            rc = rf_args_ok(e, d.nsamp, d.n, d.gauss, d.fsamp, d.waveno);
        } else if (!rc && d.kind == BH_TARGET_USER) {
            /* likelihood-only target */
        } else if (!rc) {
            rc = fail(e, BH_EINVAL, "unknown target kind");
        }
        if (!rc && d.law == BH_LAW_NOCORR_SCALED && !d.yerr) rc = fail(e, BH_EINVAL, "scaled-error law needs yerr");
        if (!rc && d.law == BH_LAW_GAUSS && !d.rinv) rc = fail(e, BH_EINVAL, "Gauss law needs rinv");
        const size_t nb = (size_t)d.n * sizeof(double);
        if (!rc) rc = ensure(e, t.yobs, nb);
        if (!rc && hipMemcpy(t.yobs.p, d.yobs, nb, hipMemcpyHostToDevice) != hipSuccess) rc = fail(e, BH_EHIP, "copy yobs");
        if (!rc && d.kind == BH_TARGET_SWD) {
            rc = ensure(e, t.x, nb);
            if (!rc && hipMemcpy(t.x.p, d.x, nb, hipMemcpyHostToDevice) != hipSuccess) rc = fail(e, BH_EHIP, "copy x");
            t.kfwd = d.n;
            if (!rc) {
                t.x_host.assign(d.x, d.x + d.n);
                t.xid = period_id(tmp, i);
            }
            if (!rc && d.n > BH_MAX_PERIODS) {
                // surf96_modsw.py:35-43: np.linspace(min, max, 60), velocities interpolated back (:119-122)
                double lo = d.x[0], hi = d.x[0];
                for (int k = 1; k < d.n; ++k) {
                    lo = d.x[k] < lo ? d.x[k] : lo;
                    hi = d.x[k] > hi ? d.x[k] : hi;
                }
                double g[BH_MAX_PERIODS];
                const double step = (hi - lo) / (double)(BH_MAX_PERIODS - 1);
                for (int k = 0; k < BH_MAX_PERIODS; ++k) g[k] = (double)k * step + lo; // numpy.linspace
                g[BH_MAX_PERIODS - 1] = hi;
                t.kfwd = BH_MAX_PERIODS;
                rc = ensure(e, t.x60, sizeof(g));
                if (!rc && hipMemcpy(t.x60.p, g, sizeof(g), hipMemcpyHostToDevice) != hipSuccess) rc = fail(e, BH_EHIP, "copy x60");
            }
        }
        if (!rc && d.law == BH_LAW_NOCORR_SCALED) { // Targets.py:124-128
            std::vector<double> se((size_t)d.n);
            t.logdet_extra = scaled_errors(d.yerr, d.n, se.data());
            rc = ensure(e, t.yerr_scaled, nb);
            if (!rc && hipMemcpy(t.yerr_scaled.p, se.data(), nb, hipMemcpyHostToDevice) != hipSuccess) rc = fail(e, BH_EHIP, "copy yerr");
        }
        if (!rc && d.law == BH_LAW_GAUSS) {
            t.logdet_extra = d.logdet_r;
            rc = ensure(e, t.rinv, nb * (size_t)d.n);
            if (!rc && hipMemcpy(t.rinv.p, d.rinv, nb * (size_t)d.n, hipMemcpyHostToDevice) != hipSuccess) rc = fail(e, BH_EHIP, "copy rinv");
        }
        if (rc) {
            for (auto &u : tmp) release_target(u);
            return rc;
        }
        // the engine keeps no host pointers
        t.d.x = t.d.yobs = t.d.yerr = t.d.rinv = nullptr;
        off += d.n;
    }
    e->targets.swap(tmp);
    e->nt = nt;
    e->ldy = off;
    e->err_t_nt = e->err_t_B = -1;
    return BH_OK;
}

int bh_targets_set_ellip(bh_engine *e, int t, int K, const double *periods, int nsteps, int is_signed, int zh)
{
    if (!e) return BH_EINVAL;
    if (t < 0 || t >= e->nt) return fail(e, BH_EINVAL, "bh_targets_set_ellip: no such target (bh_targets_set)");
    if (e->sites.nsites > 0) return fail(e, BH_EINVAL, "bh_targets_set_ellip: a site table is in force (call it between bh_targets_set and bh_sites_set*)");
    TargetHost &T = e->targets[(size_t)t];
    if (T.d.kind != BH_TARGET_USER) return fail(e, BH_EINVAL, "bh_targets_set_ellip: the target is not a BH_TARGET_USER");
    if (K != T.d.n) return fail(e, BH_EINVAL, "bh_targets_set_ellip: K differs from the target's n");
    if (K < 1 || K > BH_MAX_PERIODS) return fail(e, BH_EINVAL, "bh_targets_set_ellip: K must be 1..60");
    if (!periods) return fail(e, BH_EINVAL, "bh_targets_set_ellip: null periods");
    for (int k = 0; k < K; ++k)
        if (!std::isfinite(periods[k]) || !(periods[k] > 0.0)) return fail(e, BH_EINVAL, "bh_targets_set_ellip: a period that is not finite and positive");
    if (nsteps < 0 || nsteps > 3) return fail(e, BH_EINVAL, "bh_targets_set_ellip: nsteps must be 0..3");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    int rc = ensure(e, T.x, (size_t)K * sizeof(double));
    if (rc) return rc;
    HIPCHK(e, hipMemcpy(T.x.p, periods, (size_t)K * sizeof(double), hipMemcpyHostToDevice));
    T.x_host.assign(periods, periods + K);
    T.xid = period_id(e->targets, t, e->nt);
    T.ell_nsteps = nsteps; T.ell_signed = is_signed != 0; T.ell_zh = zh != 0;
    T.d.kind = BH_TARGET_ELLIP;
    T.d.iwave = BH_WAVE_RAYLEIGH; T.d.igr = BH_VEL_PHASE; T.d.mode = 1; T.d.flsph = 0; // (what its own search runs)
    T.kfwd = K;
    e->err_t_nt = e->err_t_B = -1;
    return BH_OK;
}

} // extern "C"

namespace {

// A BH_HOST call: la's noise, logL, misfits and err, the caller's host arrays, become the engine's staging buffers, with the
// noise copied in
int stage_like_io(bh_engine *e, hipStream_t st, LikeKernelArgs &la)
{
    const int B = la.B, nt = la.nt;
    int rc;
    if ((rc = ensure(e, e->noise, (size_t)B * 2 * nt * sizeof(double)))) return rc;
    if ((rc = ensure(e, e->logL, (size_t)B * sizeof(double)))) return rc;
    if ((rc = ensure(e, e->misfits, (size_t)B * (nt + 1) * sizeof(double)))) return rc;
    if ((rc = ensure(e, e->errb, (size_t)B * sizeof(int32_t)))) return rc;
    HIPCHK(e, hipMemcpyAsync(e->noise.p, la.noise, (size_t)B * 2 * nt * sizeof(double), hipMemcpyHostToDevice, st));
    la.noise = (const double *)e->noise.p; la.logL = (double *)e->logL.p;
    la.misfits = (double *)e->misfits.p; la.err = (int32_t *)e->errb.p;
    return BH_OK;
}

// ... and its results go back to the caller's host arrays (enqueued: the caller synchronises)
int return_like_io(bh_engine *e, hipStream_t st, const LikeKernelArgs &la, double *logL, double *misfits, int32_t *err)
{
    HIPCHK(e, hipMemcpyAsync(logL, la.logL, (size_t)la.B * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipMemcpyAsync(misfits, la.misfits, (size_t)la.B * (la.nt + 1) * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipMemcpyAsync(err, la.err, (size_t)la.B * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    return BH_OK;
}

// One fused call as its steps see it: the stream, the model arrays and where the kernels read and write.  As the caller gave
// them until stage_eval_inputs and size_eval_workspaces have run, device memory from then on.
struct EvalCall {
    hipStream_t st;
    int Lmax;
    Staged m;
    ptrdiff_t sl, sb;
    const int32_t *site; // of every model; null: bh_evaluate_batch
    double *ymod;        // [B][ldy] synthetics; null: the caller asked for none (the engine's workspace takes them)
    LikeKernelArgs la;   // the likelihood launch: B, nt, ldy, noise, logL, misfits, err; ymod and err_t once sized (t[]: run_like)
};

int eval_args_ok(bh_engine *e, const EvalPlan &p, bool host, const EvalCall &c)
{
    if (p.nt < 1) return fail(e, BH_EINVAL, "no targets registered (bh_targets_set)");
    if (p.sites.refusal != REFUSE_NONE) return fail(e, p.sites.code, bh_site_refusal_text(p.sites.refusal)); // (the first that holds: bh_plan_sites)
    if (!c.m.nlay || !c.m.h || !c.m.vp || !c.m.vs || !c.la.noise || !c.la.logL || !c.la.misfits || !c.la.err) return fail(e, BH_EINVAL, "null argument");
    if (c.site && host)
        for (int b = 0; b < p.B; ++b)
            if (c.site[b] < 0 || c.site[b] >= e->sites.nsites) return fail(e, BH_EINVAL, "site index out of range (bh_sites_set)");
    return BH_OK;
}

// A BH_HOST call's arrays go to the engine's staging buffers; the density where the caller gave none
int stage_eval_inputs(bh_engine *e, bool host, int B, EvalCall &c)
{
    int rc;
    if (host) {
        if ((rc = stage_models(e, B, c.Lmax, c.sl, c.sb, c.m))) return rc;
        if ((rc = stage_like_io(e, c.st, c.la))) return rc;
        if (c.site) {
            if ((rc = ensure(e, e->sites.idx, (size_t)B * sizeof(int32_t)))) return rc;
            HIPCHK(e, hipMemcpyAsync(e->sites.idx.p, c.site, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, c.st));
            c.site = (const int32_t *)e->sites.idx.p;
        }
        c.ymod = nullptr;
    }
    if (!c.m.rho) { // rho = 0.32 vp + 0.77 (Targets.py:319)
        const size_t nel = span_elems(B, c.Lmax, c.sl, c.sb);
        if ((rc = ensure(e, e->rho, nel * sizeof(double)))) return rc;
        hipLaunchKernelGGL(rho_from_vp_kernel, dim3((unsigned)((nel + 255) / 256)), dim3(256), 0, c.st, nel, c.m.vp, (double *)e->rho.p);
        c.m.rho = (const double *)e->rho.p;
    }
    return BH_OK;
}

// The workspaces whose size follows from the plan: the synthetics, the failure flags, the 60-period grids' velocities and the
// fused likelihoods' sums
int size_eval_workspaces(bh_engine *e, const EvalPlan &p, EvalCall &c)
{
    int rc;
    if (!c.ymod) {
        if ((rc = ensure(e, e->ymod, (size_t)p.B * p.ldy * sizeof(double)))) return rc;
        c.ymod = (double *)e->ymod.p;
    }
    const size_t cap0 = e->err_t.cap;
    if ((rc = ensure(e, e->err_t, (size_t)p.nt * p.B * sizeof(int32_t)))) return rc;
    if (e->err_t.cap != cap0) e->err_t_nt = e->err_t_B = -1; // a new buffer: not zeroed yet
    c.la.ymod = c.ymod; c.la.err_t = (const int32_t *)e->err_t.p;
    for (int t = 0; t < p.nt; ++t) {
        TargetHost &T = e->targets[(size_t)t];
        if (p.role[t] == ROLE_SWD60 && (rc = ensure(e, T.vel60, (size_t)p.B * T.kfwd * sizeof(double)))) return rc;
        if (p.rf_fused[t] && (rc = ensure(e, T.sums, (size_t)p.B * 4 * sizeof(double)))) return rc;
        if (p.role[t] == ROLE_ELLIP && p.ell_source[t] < 0 && (rc = ensure(e, T.ell_vel, (size_t)p.B * T.d.n * sizeof(double)))) return rc;
    }
    return BH_OK;
}

// The forward models of the plan: fork -> [dispersion | gate, receiver functions] -> join
int run_forward(bh_engine *e, const EvalPlan &p, const EvalCall &c)
{
    const int B = p.B, nt = p.nt, ldy = p.ldy;
    hipStream_t st = c.st, rst = p.fork ? e->aux : st;
    int rc;
    SwdJob jobs[BH_MAX_TARGETS];
    int njobs = 0;
    const SiteTable &S = e->sites;
    const SitePlan &sp = p.sites;
    const SwdSiteXArgs xtab{c.site, S.nsites, nt, ldy, (const int32_t *)S.xn.p, (const double *)S.xper.p, {}, {}};
    for (int t = 0; t < nt; ++t) {
        const TargetHost &T = e->targets[(size_t)t];
        const bh_target_desc &d = T.d;
        int32_t *errp = (int32_t *)e->err_t.p + (size_t)t * B;
        if (p.role[t] == ROLE_SWD) {
            jobs[njobs++] = SwdJob{d.n, d.iwave, d.igr, ldy, (const double *)T.x.p, c.ymod + T.off, errp, d.mode, d.flsph};
            if (sp.x_table) jobs[njobs - 1].sx = SwdSiteJob{&xtab, t, T.off, sp.x_all};
        } else if (p.role[t] == ROLE_SWD60) {
            jobs[njobs++] = SwdJob{T.kfwd, d.iwave, d.igr, T.kfwd, (const double *)T.x60.p, (double *)T.vel60.p, errp, d.mode, d.flsph};
        }
    }
    // (the ellipticity targets' own searches come after the dispersion targets' jobs: those keep their places in the launch and
    // in the guard's statistics.  Under a period table the job reads the table's column of its target, which holds the periods
    // every site shares.)
    for (int t = 0; t < nt; ++t) {
        if (p.role[t] != ROLE_ELLIP || p.ell_source[t] >= 0) continue;
        const TargetHost &T = e->targets[(size_t)t];
        jobs[njobs++] = SwdJob{T.d.n, BH_WAVE_RAYLEIGH, BH_VEL_PHASE, T.d.n, (const double *)T.x.p, (double *)T.ell_vel.p,
                               (int32_t *)e->err_t.p + (size_t)t * B, 1, 0};
        if (sp.x_table) jobs[njobs - 1].sx = SwdSiteJob{&xtab, t, T.off, sp.x_all};
    }
    // per-target failure flags [nt][B]: the dispersion kernels write every entry of their target's row on every call,
    // nothing writes the rows of the other targets -- they are zeroed once per (nt, B) layout, not once per call; by the dispersion
    // call's ordering launch where its plan has one (the receiver-function launches beside it neither read nor write the flags)
    const SwdPlan swp = plan_swd_call(e, B, c.Lmax, c.m, njobs, jobs);
    SwdFills fills{};
    if (p.err_zero_always || e->err_t_nt != nt || e->err_t_B != B) {
        if (swp.prologue) {
            fills.err = (int32_t *)e->err_t.p;
            fills.nerr = nt * B;
        } else {
            HIPCHK(e, hipMemsetAsync(e->err_t.p, 0, (size_t)nt * B * sizeof(int32_t), st));
        }
        e->err_t_nt = nt;
        e->err_t_B = B;
    }
    if (p.fork && (rc = wait_for(e, e->ev_fork, st, e->aux))) return rc;
    if (e->started != nullptr && e->started_expected > 0x70000000u) { // (the counter is cumulative: rewind it long before it wraps)
        HIPCHK(e, hipStreamSynchronize(st));
        HIPCHK(e, hipStreamSynchronize(e->aux));
        HIPCHK(e, hipMemset(e->started, 0, sizeof(unsigned)));
        e->started_expected = 0;
    }
    SwdLaunchInfo swd{};
    if ((rc = launch_swd_jobs(e, st, B, c.Lmax, c.m, c.sl, c.sb, njobs, jobs, swp, fills, p.prio_low, &swd))) return rc;
    const bool gate = p.want_gate && swd.workgroups > 0;
    if (gate)
        HIPCHK(e, hipStreamWaitValue32(e->aux, e->started, e->started_expected - swd.workgroups + gate_need(swd), hipStreamWaitValueGte, 0xffffffffu));
    for (int t = 0; t < nt; ++t) {
        TargetHost &T = e->targets[(size_t)t];
        const bh_target_desc &d = T.d;
        if (p.role[t] == ROLE_SWD60)
            bh_launch_interp(B, T.kfwd, (const double *)T.x60.p, (const double *)T.vel60.p, T.kfwd, d.n,
                             (const double *)T.x.p, c.ymod + T.off, ldy, st);
        if (p.role[t] != ROLE_RF) continue;
        RfJob job{d.p_s_per_deg, d.gauss, d.nsamp, d.fsamp, d.tshift, d.nsv, d.waveno, d.n, c.ymod + T.off, ldy,
                  p.rf_fused[t] ? (const double *)T.yobs.p : nullptr, p.rf_fused[t] ? (double *)T.sums.p : nullptr, rf_build(sp), RfSiteTArgs{}};
        RfSiteTArgs &rs = job.sites; // (column t of the tables in force)
        if (sp.rf_table) {
            rs.site = c.site; rs.nsites = S.nsites; rs.ld = nt;
            rs.p = (const double *)S.p.p + t; rs.nsv = (const double *)S.nsv.p + t;
        }
        if (sp.missing || sp.rf_axis) rs.n = (const int32_t *)S.xn.p + t;
        if (sp.rf_axis) {
            rs.axis = (const RfAxisRec *)S.axis.p + t;
            rs.nsamp_max = S.t[t].axis_nsamp_max;
        }
        if ((rc = launch_rf(e, rst, B, c.Lmax, c.m, c.sl, c.sb, job, p.fork, gate))) return rc;
    }
    // The ellipticities, on the call's stream behind the dispersion launches (the guard's re-run included: the velocities are
    // final) and before the join.  Row t of err_t is written in full on every call: by the target's own search, or by a copy of
    // the row of the target whose search it shares; the kernel ORs its own failures into it.
    for (int t = 0; t < nt; ++t) {
        if (p.role[t] != ROLE_ELLIP) continue;
        const TargetHost &T = e->targets[(size_t)t];
        const int j = p.ell_source[t];
        int32_t *row = (int32_t *)e->err_t.p + (size_t)t * B;
        if (j >= 0)
            HIPCHK(e, hipMemcpyAsync(row, (const int32_t *)e->err_t.p + (size_t)j * B, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        EllipFusedArgs a{};
        a.B = B; a.Lmax = c.Lmax; a.K = T.d.n; a.nsteps = T.ell_nsteps; a.is_signed = T.ell_signed; a.zh = T.ell_zh;
        a.nlay = c.m.nlay; a.h = c.m.h; a.vp = c.m.vp; a.vs = c.m.vs; a.rho = c.m.rho;
        a.sl = c.sl; a.sb = c.sb;
        a.periods = (const double *)T.x.p;
        a.vel = j >= 0 ? c.ymod + e->targets[(size_t)j].off : (const double *)T.ell_vel.p;
        a.ldvel = j >= 0 ? ldy : T.d.n;
        a.y = c.ymod + T.off; a.ldy = ldy;
        a.err_row = row;
        bh_launch_ellip_fused(a, st);
    }
    return p.fork ? wait_for(e, e->ev_join, e->aux, st) : BH_OK;
}

// The likelihood of every model from the synthetics (or the sums of the targets in `fused`) and the failure flags, by the launcher
// and the tables of the site plan sp.  site: of every model, or null (LIKE_PLAIN)
int run_like(bh_engine *e, hipStream_t st, LikeKernelArgs la, const bool *fused, const SitePlan &sp, const int32_t *site)
{
    const SiteTable &S = e->sites;
    int rc;
    for (int t = 0; t < la.nt; ++t)
        if ((rc = prepare_like_target(e, st, la.B, la.ldy, la.ymod, t, la.t[t], fused[t], site, sp.gauss[t]))) return rc;
    LikeSiteXArgs lx{};
    lx.site = site; lx.nsites = S.nsites; lx.yobs = (const double *)S.yobs.p; lx.yerr_scaled = (const double *)S.yerr.p;
    lx.logdet_extra = (const double *)S.logdet.p;
    lx.n = (const int32_t *)(sp.desc_counts ? S.desc_n.p : S.xn.p);
    LikeClassArgs lc{};
    if (sp.like == LIKE_SITES_C || sp.like == LIKE_SITES_L)
        for (int t = 0; t < la.nt; ++t) {
            if (sp.gauss[t] != GAUSS_CLASSES || e->targets[(size_t)t].d.law != BH_LAW_GAUSS) continue;
            lc.class_of[t] = (const int32_t *)S.t[t].class_of.p;
            lc.rinv[t] = (const double *)S.t[t].rinv.p;
            lc.logdet[t] = (const double *)S.t[t].logdet.p;
        }
    ev_begin(e, 2, st);
    if (sp.like == LIKE_SITES_L) { // (the law-1 tables formed by the table's laws; a law table comes with a count table)
        lx.yerr_scaled = (const double *)S.law_yerr.p;
        lx.logdet_extra = (const double *)S.law_logdet.p;
        bh_launch_like_sites_l(la, lx, lc, LikeLawArgs{(const int32_t *)S.law.p}, st);
    } else if (sp.like == LIKE_SITES_C) bh_launch_like_sites_c(la, lx, lc, st);
    else if (sp.like == LIKE_SITES_M) bh_launch_like_sites_m(la, lx, st); // (counts of which some may be 0)
    else if (sp.like == LIKE_SITES_X) bh_launch_like_sites_x(la, lx, st); // (a site's own sample counts)
    else if (sp.like == LIKE_SITES) bh_launch_like_sites(la, lx, st);
    else bh_launch_like(la, st);
    ev_end(e, 2, st);
    return BH_OK;
}

// bh_evaluate_batch (site == nullptr: exactly its launches) and bh_evaluate_sites (site = the caller's site index per model):
// validate, stage the inputs, size the workspaces, run the plan's forward models and likelihood, copy the results back.
// (The plan is pure and comes first: the validation refuses a call whose plan holds a refusal.)
int evaluate(bh_engine *e, int memspace, void *stream, int B, int Lmax, const int32_t *nlay, const double *h, const double *vp,
             const double *vs, const double *rho, ptrdiff_t sl, ptrdiff_t sb, const int32_t *site, const double *noise,
             double *logL, double *misfits, int32_t *err, double *ymod)
{
    int rc;
    if ((rc = check_models(e, B, Lmax, sl, sb))) return rc;
    const bool host = (memspace != BH_DEVICE);
    const EvalPlan p = plan_eval(e, B, site != nullptr, ymod != nullptr);
    LikeKernelArgs la{};
    la.B = B; la.nt = p.nt; la.ldy = p.ldy; la.noise = noise; la.logL = logL; la.misfits = misfits; la.err = err;
    EvalCall c{(!host && stream) ? (hipStream_t)stream : e->stream, Lmax, Staged{nlay, h, vp, vs, rho, nullptr, nullptr}, sl, sb, site, ymod, la};
    if ((rc = eval_args_ok(e, p, host, c))) return rc;
    if (B == 0) return BH_OK;
    HIPCHK(e, hipSetDevice(e->device));
    if ((rc = stage_eval_inputs(e, host, B, c)) || (rc = size_eval_workspaces(e, p, c))) return rc;
    call_begin(e, c.st);
    if ((rc = run_forward(e, p, c)) || (rc = run_like(e, c.st, c.la, p.rf_fused, p.sites, c.site))) return rc;
    call_end(e, c.st);
    HIPCHK(e, hipGetLastError());
    if (!host) return BH_OK;
    if ((rc = return_like_io(e, c.st, c.la, logL, misfits, err))) return rc;
    if (ymod) HIPCHK(e, hipMemcpyAsync(ymod, c.ymod, (size_t)B * p.ldy * sizeof(double), hipMemcpyDeviceToHost, c.st));
    HIPCHK(e, hipStreamSynchronize(c.st));
    return BH_OK;
}

} // namespace

extern "C" {

int bh_evaluate_batch(bh_engine *e, int memspace, void *stream, int B, int Lmax,
                      const int32_t *nlay, const double *h, const double *vp, const double *vs,
                      const double *rho, ptrdiff_t sl, ptrdiff_t sb, const double *noise,
                      double *logL, double *misfits, int32_t *err, double *ymod)
{
    return evaluate(e, memspace, stream, B, Lmax, nlay, h, vp, vs, rho, sl, sb, nullptr, noise, logL, misfits, err, ymod);
}

// bh_sites_set (n == null: every site has the descriptors' counts) and bh_sites_set_x (n[s * nt + t] samples of site s for
// target t: yobs, yerr and the scaled-error tables are formed over a site's own samples; the columns beyond them hold 0 / 1)
static int sites_register(bh_engine *e, int nsites, const int32_t *n, const double *yobs, const double *yerr)
{
    const int nt = e->nt, ldy = e->ldy;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    SiteTable &tab = e->sites;
    tab.drop(PART_COUNTS);
    const size_t S = (size_t)nsites;
    std::vector<double> se(S * ldy, 1.0), ld(S * nt, 0.0), yo;
    if (n) yo.assign(S * ldy, 0.0);
    for (size_t s = 0; s < S; ++s)
        for (int t = 0; t < nt; ++t) {
            const TargetHost &T = e->targets[(size_t)t];
            const int ns = n ? n[s * nt + t] : T.d.n;
            ld[s * nt + t] = T.logdet_extra;
            if (T.d.law == BH_LAW_NOCORR_SCALED)
                ld[s * nt + t] = scaled_errors(yerr + s * ldy + T.off, ns, se.data() + s * ldy + T.off);
            if (n) std::copy(yobs + s * ldy + T.off, yobs + s * ldy + T.off + ns, yo.data() + s * ldy + T.off);
        }
    int rc;
    if ((rc = ensure(e, tab.yobs, S * ldy * sizeof(double))) || (rc = ensure(e, tab.yerr, S * ldy * sizeof(double))) ||
        (rc = ensure(e, tab.logdet, S * nt * sizeof(double)))) {
        tab.drop(PART_COUNTS);
        return rc;
    }
    if (hipMemcpy(tab.yobs.p, n ? yo.data() : yobs, S * ldy * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(tab.yerr.p, se.data(), S * ldy * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(tab.logdet.p, ld.data(), S * nt * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
        tab.drop(PART_COUNTS);
        return fail(e, BH_EHIP, "copy site table");
    }
    tab.nsites = nsites;
    tab.level = SITES_SHARED;
    return BH_OK;
}

int bh_sites_set(bh_engine *e, int nsites, const double *yobs, const double *yerr)
{
    if (!e) return BH_EINVAL;
    if (e->nt < 1) return fail(e, BH_EINVAL, "no targets registered (bh_targets_set)");
    if (nsites < 1 || !yobs) return fail(e, BH_EINVAL, "bh_sites_set needs nsites >= 1 and yobs");
    bool scaled = false;
    for (const auto &T : e->targets) scaled = scaled || T.d.law == BH_LAW_NOCORR_SCALED;
    if (scaled && !yerr) return fail(e, BH_EINVAL, "a BH_LAW_NOCORR_SCALED target needs yerr of every site");
    return sites_register(e, nsites, nullptr, yobs, yerr);
}

// The count tables, bh_sites_set_x ... bh_sites_set_axes (who: the entry point's name, for the messages; level: what it registers,
// SITES_X ... SITES_AXES).  Every level admits one thing more than the one before it, named below where it is checked.
static int sites_register_x(bh_engine *e, const char *who, SiteLevel level, int nsites, const int32_t *n, const double *x, const double *yobs, const double *yerr)
{
    if (!e) return BH_EINVAL;
    const std::string w(who);
    if (e->nt < 1) return fail(e, BH_EINVAL, "no targets registered (bh_targets_set)");
    if (nsites < 1 || !n || !x || !yobs) return fail(e, BH_EINVAL, (w + " needs nsites >= 1, n, x and yobs").c_str());
    const int nt = e->nt, ldy = e->ldy;
    bool scaled = false;
    for (const auto &T : e->targets) scaled = scaled || T.d.law == BH_LAW_NOCORR_SCALED;
    if (scaled && !yerr) return fail(e, BH_EINVAL, "a BH_LAW_NOCORR_SCALED target needs yerr of every site");
    const size_t S = (size_t)nsites;
    const bool admits_any_dispersion = level >= SITES_X_ALL;        // per-site periods and counts on group-velocity and higher-mode targets
    const bool admits_absent = level >= SITES_MISSING;              // a count of 0 -- the site lacks the target -- but every site has a target and every target a site
    const bool admits_absent_gauss = level >= SITES_MISSING_GAUSS;  // ... on a Gauss-law target as well
    const bool admits_rf_counts = level >= SITES_AXES;              // a receiver function's count may be 0 or 1 .. its descriptor's n
    if (admits_absent) {
        for (size_t s = 0; s < S; ++s) {
            bool any = false;
            for (int t = 0; t < nt; ++t) any = any || n[s * nt + t] != 0;
            if (!any) return fail(e, BH_EINVAL, (w + ": a site with no target (every count 0)").c_str());
        }
        for (int t = 0; t < nt; ++t) {
            bool any = false, lacks = false;
            for (size_t s = 0; s < S; ++s) {
                any = any || n[s * nt + t] != 0;
                lacks = lacks || n[s * nt + t] == 0;
            }
            if (!any) return fail(e, BH_EINVAL, (w + ": a target no site has (every count 0)").c_str());
            if (lacks && !admits_absent_gauss && e->targets[(size_t)t].d.law == BH_LAW_GAUSS)
                return fail(e, BH_EUNSUPPORTED, (w + ": a Gauss-law target that a site lacks (the contraction gathers every site's rows)").c_str());
        }
    }
    for (int t = 0; t < nt; ++t) {
        const TargetHost &T = e->targets[(size_t)t];
        const bh_target_desc &d = T.d;
        if (d.kind != BH_TARGET_SWD) { // (a receiver function's x is its descriptor's time axis: shared, but for bh_sites_set_axes)
            for (size_t s = 0; s < S; ++s) {
                if (admits_rf_counts && d.kind == BH_TARGET_RF && n[s * nt + t] >= 0 && n[s * nt + t] <= d.n) continue;
                if (admits_rf_counts && d.kind == BH_TARGET_RF) return fail(e, BH_EINVAL, (w + ": a receiver function's sample count is below 0 or above its descriptor's n (the capacity)").c_str());
                if (d.kind == BH_TARGET_ELLIP && n[s * nt + t] == 0) return fail(e, BH_EUNSUPPORTED, (w + ": an ellipticity target that a site lacks").c_str());
                if (d.kind == BH_TARGET_ELLIP && n[s * nt + t] == d.n && std::memcmp(T.x_host.data(), x + s * ldy + T.off, (size_t)d.n * sizeof(double)) != 0)
                    return fail(e, BH_EINVAL, (w + ": an ellipticity target's periods differ from its registered ones (every site shares them)").c_str());
                if (n[s * nt + t] != d.n && !(admits_absent && n[s * nt + t] == 0)) return fail(e, BH_EINVAL, (w + ": the sample count of a target that is no dispersion curve differs from its descriptor's").c_str());
            }
            continue;
        }
        if (d.law == BH_LAW_GAUSS) return fail(e, BH_EINVAL, (w + ": a dispersion target with the Gauss law (its R^-1 depends on the sample count)").c_str());
        if (T.kfwd != d.n) return fail(e, BH_EUNSUPPORTED, (w + ": a dispersion target of more than 60 periods (the interpolation path)").c_str());
        for (size_t s = 0; s < S; ++s) {
            const int ns = n[s * nt + t];
            if (admits_absent && ns == 0) continue; // (the site lacks this curve)
            if (ns < 1 || ns > d.n) return fail(e, BH_EINVAL, (w + ": a site's period count is below 1 or above the descriptor's n (the capacity)").c_str());
            for (int i = 0; i < ns; ++i) {
                const double v = x[s * ldy + T.off + i];
                if (!std::isfinite(v) || !(v > 0.0)) return fail(e, BH_EINVAL, (w + ": a period that is not finite and positive").c_str());
            }
        }
        if (!admits_any_dispersion && (d.igr != BH_VEL_PHASE || d.mode > 1)) { // group velocities, higher modes: only with the descriptor's periods at every site
            std::vector<double> x0((size_t)d.n);
            HIPCHK(e, hipSetDevice(e->device));
            HIPCHK(e, hipMemcpy(x0.data(), T.x.p, (size_t)d.n * sizeof(double), hipMemcpyDeviceToHost));
            for (size_t s = 0; s < S; ++s)
                if (n[s * nt + t] != d.n || std::memcmp(x0.data(), x + s * ldy + T.off, (size_t)d.n * sizeof(double)) != 0)
                    return fail(e, BH_EUNSUPPORTED, (w + ": per-site periods on a group-velocity or higher-mode target").c_str());
        }
    }
    int rc = sites_register(e, nsites, n, yobs, yerr);
    if (rc) return rc;
    std::vector<double> xs(S * ldy, 0.0);
    for (size_t s = 0; s < S; ++s)
        for (int t = 0; t < nt; ++t) {
            const TargetHost &T = e->targets[(size_t)t];
            if (T.d.kind == BH_TARGET_SWD || T.d.kind == BH_TARGET_ELLIP) std::copy(x + s * ldy + T.off, x + s * ldy + T.off + n[s * nt + t], xs.data() + s * ldy + T.off);
        }
    SiteTable &tab = e->sites;
    if ((rc = ensure(e, tab.xn, S * nt * sizeof(int32_t))) || (rc = ensure(e, tab.xper, S * ldy * sizeof(double)))) {
        tab.drop(PART_COUNTS);
        return rc;
    }
    if (hipMemcpy(tab.xn.p, n, S * nt * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(tab.xper.p, xs.data(), S * ldy * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
        tab.drop(PART_COUNTS);
        return fail(e, BH_EHIP, "copy site table");
    }
    tab.level = level;
    tab.xn_host.assign(n, n + S * nt);
    for (int t = 0; t < nt; ++t)
        for (size_t s = 0; s < S; ++s)
            if (n[s * nt + t] == 0) tab.t[t].lacks = true;
            else if (e->targets[(size_t)t].d.kind == BH_TARGET_RF && n[s * nt + t] != e->targets[(size_t)t].d.n) tab.t[t].rf_own_counts = true;
    return BH_OK;
}

int bh_sites_set_x(bh_engine *e, int nsites, const int32_t *n, const double *x, const double *yobs, const double *yerr)
{
    return sites_register_x(e, "bh_sites_set_x", SITES_X, nsites, n, x, yobs, yerr);
}

int bh_sites_set_x_all(bh_engine *e, int nsites, const int32_t *n, const double *x, const double *yobs, const double *yerr)
{
    return sites_register_x(e, "bh_sites_set_x_all", SITES_X_ALL, nsites, n, x, yobs, yerr);
}

int bh_sites_set_missing(bh_engine *e, int nsites, const int32_t *n, const double *x, const double *yobs, const double *yerr)
{
    return sites_register_x(e, "bh_sites_set_missing", SITES_MISSING, nsites, n, x, yobs, yerr);
}

int bh_sites_set_missing_gauss(bh_engine *e, int nsites, const int32_t *n, const double *x, const double *yobs, const double *yerr)
{
    return sites_register_x(e, "bh_sites_set_missing_gauss", SITES_MISSING_GAUSS, nsites, n, x, yobs, yerr);
}

int bh_sites_set_axes(bh_engine *e, int nsites, const int32_t *n, const double *x, const double *yobs, const double *yerr)
{
    return sites_register_x(e, "bh_sites_set_axes", SITES_AXES, nsites, n, x, yobs, yerr);
}

int bh_sites_set_gauss(bh_engine *e, int target, int nsites, int nclass, const int32_t *class_of, const double *rinv, const double *logdet_r)
{
    if (!e) return BH_EINVAL;
    if (e->sites.nsites < 1) return fail(e, BH_EINVAL, "no site table registered (bh_sites_set)");
    if (nsites != e->sites.nsites) return fail(e, BH_EINVAL, "bh_sites_set_gauss: nsites differs from the site table's");
    if (target < 0 || target >= e->nt || e->targets[(size_t)target].d.law != BH_LAW_GAUSS)
        return fail(e, BH_EINVAL, "bh_sites_set_gauss: not a BH_LAW_GAUSS target");
    if (nclass < 1) return fail(e, BH_EINVAL, "bh_sites_set_gauss: nclass must be at least 1");
    if (!class_of || !rinv || !logdet_r) return fail(e, BH_EINVAL, "null argument");
    const TargetHost &T = e->targets[(size_t)target];
    SiteTable &tab = e->sites;
    SiteTarget &G = tab.t[target];
    const size_t nn = (size_t)T.d.n * (size_t)T.d.n, S = (size_t)nsites, nt = (size_t)e->nt;
    if ((size_t)nclass > BH_SITES_GAUSS_MAXBYTES / sizeof(double) / nn)
        return fail(e, BH_EUNSUPPORTED, "bh_sites_set_gauss: the matrices take more than BH_SITES_GAUSS_MAXBYTES (1 GiB)");
    if (nclass > BH_SITES_GAUSS_MAXCLASSES) return fail(e, BH_EUNSUPPORTED, "bh_sites_set_gauss: more than BH_SITES_GAUSS_MAXCLASSES (4096) classes");
    for (size_t s = 0; s < S; ++s) {
        const int c = class_of[s];
        if (c < -1 || c >= nclass) return fail(e, BH_EINVAL, "bh_sites_set_gauss: a class index outside [-1, nclass)");
        const bool has = tab.xn_host.empty() || tab.xn_host[s * nt + (size_t)target] != 0; // (bh_sites_set: every site has every target)
        if (has && tab.laws) { // (bh_sites_set_laws: a class exactly for the sites under the Gauss law on this target)
            const bool gauss = tab.law_host[s * nt + (size_t)target] == BH_LAW_GAUSS;
            if (gauss && c < 0) return fail(e, BH_EINVAL, "bh_sites_set_gauss: class -1 for a site under the Gauss law on the target (bh_sites_set_laws)");
            if (!gauss && c >= 0) return fail(e, BH_EINVAL, "bh_sites_set_gauss: a class for a site under another law than BH_LAW_GAUSS on the target (bh_sites_set_laws)");
            continue;
        }
        if (has && c < 0) return fail(e, BH_EINVAL, "bh_sites_set_gauss: class -1 for a site that has the target");
        if (!has && c >= 0) return fail(e, BH_EINVAL, "bh_sites_set_gauss: a class for a site that lacks the target (count 0)");
    }
    for (size_t i = 0; i < (size_t)nclass * nn; ++i)
        if (!std::isfinite(rinv[i])) return fail(e, BH_EINVAL, "bh_sites_set_gauss: a non-finite value in rinv");
    for (int c = 0; c < nclass; ++c)
        if (!std::isfinite(logdet_r[c])) return fail(e, BH_EINVAL, "bh_sites_set_gauss: a non-finite value in logdet_r");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    tab.drop(PART_CLASSES, target);
    int rc;
    if ((rc = ensure(e, G.rinv, (size_t)nclass * nn * sizeof(double))) || (rc = ensure(e, G.logdet, (size_t)nclass * sizeof(double))) ||
        (rc = ensure(e, G.class_of, S * sizeof(int32_t))))
        return rc;
    HIPCHK(e, hipMemcpy(G.rinv.p, rinv, (size_t)nclass * nn * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(G.logdet.p, logdet_r, (size_t)nclass * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(G.class_of.p, class_of, S * sizeof(int32_t), hipMemcpyHostToDevice));
    if (tab.level < SITES_X && !tab.desc_n.p) { // no count table in force: the likelihood build of the class calls reads the descriptors' counts
        std::vector<int32_t> cnt(S * nt);
        for (size_t s = 0; s < S; ++s)
            for (size_t t = 0; t < nt; ++t) cnt[s * nt + t] = e->targets[t].d.n;
        if ((rc = ensure(e, tab.desc_n, S * nt * sizeof(int32_t)))) return rc;
        HIPCHK(e, hipMemcpy(tab.desc_n.p, cnt.data(), S * nt * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    G.nclass = nclass;
    return BH_OK;
}

int bh_sites_set_laws(bh_engine *e, int nsites, const int32_t *law, const double *yerr)
{
    if (!e) return BH_EINVAL;
    if (e->sites.nsites < 1) return fail(e, BH_EINVAL, "no site table registered (bh_sites_set)");
    if (e->sites.level < SITES_MISSING_GAUSS)
        return fail(e, BH_EINVAL, "bh_sites_set_laws: no count table registered that accepts a Gauss-law target some site lacks (bh_sites_set_missing_gauss, bh_sites_set_axes)");
    if (nsites != e->sites.nsites) return fail(e, BH_EINVAL, "bh_sites_set_laws: nsites differs from the site table's");
    if (!law) return fail(e, BH_EINVAL, "null argument");
    const int nt = e->nt, ldy = e->ldy;
    const size_t S = (size_t)nsites;
    std::vector<int32_t> lw(S * nt, 0); // (0 where the count is 0: the caller's entry is not read)
    std::vector<double> se(S * ldy, 1.0), ld(S * nt, 0.0);
    std::vector<char> other((size_t)nt, 0);
    for (size_t s = 0; s < S; ++s)
        for (int t = 0; t < nt; ++t) {
            const TargetHost &T = e->targets[(size_t)t];
            const int ns = e->sites.xn_host[s * nt + t];
            if (ns == 0) continue; // (the site lacks the target)
            const int l = law[s * nt + t];
            if (l != BH_LAW_NOCORR && l != BH_LAW_NOCORR_SCALED && l != BH_LAW_EXP && l != BH_LAW_GAUSS)
                return fail(e, BH_EINVAL, "bh_sites_set_laws: an unknown noise law");
            if (l == BH_LAW_GAUSS && T.d.law != BH_LAW_GAUSS)
                return fail(e, BH_EINVAL, "bh_sites_set_laws: BH_LAW_GAUSS on a target whose descriptor is not BH_LAW_GAUSS (the descriptor owns the contraction's shape and workspace)");
            if (l == BH_LAW_NOCORR_SCALED) { // Targets.py:124-128, over the site's own samples
                if (!yerr) return fail(e, BH_EINVAL, "bh_sites_set_laws: a BH_LAW_NOCORR_SCALED pair needs yerr");
                for (int i = 0; i < ns; ++i) {
                    const double v = yerr[s * ldy + T.off + i];
                    if (!std::isfinite(v) || !(v > 0.0)) return fail(e, BH_EINVAL, "bh_sites_set_laws: an error that is not finite and positive under BH_LAW_NOCORR_SCALED");
                }
                ld[s * nt + t] = scaled_errors(yerr + s * ldy + T.off, ns, se.data() + s * ldy + T.off);
            }
            if (l != BH_LAW_GAUSS) other[(size_t)t] = 1;
            lw[s * nt + t] = l;
        }
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    SiteTable &tab = e->sites;
    tab.drop(PART_LAWS);
    int rc;
    if ((rc = ensure(e, tab.law, S * nt * sizeof(int32_t))) || (rc = ensure(e, tab.law_yerr, S * ldy * sizeof(double))) ||
        (rc = ensure(e, tab.law_logdet, S * nt * sizeof(double))))
        return rc;
    HIPCHK(e, hipMemcpy(tab.law.p, lw.data(), S * nt * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(tab.law_yerr.p, se.data(), S * ldy * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(tab.law_logdet.p, ld.data(), S * nt * sizeof(double), hipMemcpyHostToDevice));
    for (int t = 0; t < nt; ++t) tab.t[t].law_other = other[(size_t)t] != 0;
    tab.law_host = lw;
    tab.laws = true;
    return BH_OK;
}

int bh_sites_set_rf(bh_engine *e, int nsites, const double *p_s_per_deg, const double *nsv)
{
    if (!e) return BH_EINVAL;
    if (e->sites.nsites < 1) return fail(e, BH_EINVAL, "no site table registered (bh_sites_set)");
    if (nsites != e->sites.nsites) return fail(e, BH_EINVAL, "bh_sites_set_rf: nsites differs from the site table's");
    if (!p_s_per_deg || !nsv) return fail(e, BH_EINVAL, "null argument");
    const int nt = e->nt;
    const size_t n = (size_t)nsites * (size_t)nt;
    for (int t = 0; t < nt; ++t) {
        if (e->targets[(size_t)t].d.kind != BH_TARGET_RF) continue;
        for (int s = 0; s < nsites; ++s)
            if (!std::isfinite(p_s_per_deg[(size_t)s * nt + t]) || !std::isfinite(nsv[(size_t)s * nt + t]))
                return fail(e, BH_EINVAL, "bh_sites_set_rf: a receiver-function column holds a non-finite value");
    }
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    SiteTable &tab = e->sites;
    tab.drop(PART_RF);
    int rc;
    if ((rc = ensure(e, tab.p, n * sizeof(double))) || (rc = ensure(e, tab.nsv, n * sizeof(double)))) return rc;
    HIPCHK(e, hipMemcpy(tab.p.p, p_s_per_deg, n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(tab.nsv.p, nsv, n * sizeof(double), hipMemcpyHostToDevice));
    tab.rf = true;
    return BH_OK;
}

int bh_sites_set_rf_axis(bh_engine *e, int nsites, const int32_t *nsamp, const double *fsamp, const double *tshift, const double *gauss)
{
    if (!e) return BH_EINVAL;
    if (e->sites.nsites < 1) return fail(e, BH_EINVAL, "no site table registered (bh_sites_set)");
    if (e->sites.level < SITES_X) return fail(e, BH_EINVAL, "bh_sites_set_rf_axis: no count table registered (bh_sites_set_axes)");
    if (!e->sites.rf) return fail(e, BH_EINVAL, "bh_sites_set_rf_axis needs the table of bh_sites_set_rf (the coefficient stage finds the model's site through it)");
    if (nsites != e->sites.nsites) return fail(e, BH_EINVAL, "bh_sites_set_rf_axis: nsites differs from the site table's");
    if (!nsamp || !fsamp || !tshift || !gauss) return fail(e, BH_EINVAL, "null argument");
    const int nt = e->nt;
    const size_t S = (size_t)nsites;
    std::vector<RfAxisRec> recs(S * (size_t)nt, RfAxisRec{1.0, 0.0, 1.0, 4, 1, 3, 0}); // (other targets' and absent pairs' entries: never read)
    std::vector<int> nmax((size_t)nt, 0);
    for (int t = 0; t < nt; ++t) {
        if (e->targets[(size_t)t].d.kind != BH_TARGET_RF) continue;
        for (size_t s = 0; s < S; ++s) {
            const size_t i = s * (size_t)nt + (size_t)t;
            const int cnt = e->sites.xn_host[i];
            if (cnt == 0) continue; // (the site lacks the target)
            const int ns = nsamp[i];
            if (ns < 4 || (ns & (ns - 1)) != 0) return fail(e, BH_EINVAL, "bh_sites_set_rf_axis: nsamp must be a power of two >= 4");
            if (ns > BH_SITES_RF_AXIS_MAX_NSAMP)
                return fail(e, BH_EUNSUPPORTED, "bh_sites_set_rf_axis: nsamp above 16384 (the HBM-workspace build stays on the shared axis)");
            if (ns < cnt) return fail(e, BH_EINVAL, "bh_sites_set_rf_axis: nsamp below the site's sample count");
            if (!std::isfinite(fsamp[i]) || !(fsamp[i] > 0.0) || !std::isfinite(gauss[i]) || !(gauss[i] > 0.0))
                return fail(e, BH_EINVAL, "bh_sites_set_rf_axis: fsamp and gauss must be finite and > 0");
            if (!std::isfinite(tshift[i])) return fail(e, BH_EINVAL, "bh_sites_set_rf_axis: a non-finite tshift");
            recs[i] = bh_rf_axis_record(ns, fsamp[i], tshift[i], gauss[i]);
            nmax[(size_t)t] = std::max(nmax[(size_t)t], ns);
        }
    }
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    SiteTable &tab = e->sites;
    tab.drop(PART_RF_AXIS);
    int rc;
    if ((rc = ensure(e, tab.axis, recs.size() * sizeof(RfAxisRec)))) return rc;
    HIPCHK(e, hipMemcpy(tab.axis.p, recs.data(), recs.size() * sizeof(RfAxisRec), hipMemcpyHostToDevice));
    for (int t = 0; t < nt; ++t) tab.t[t].axis_nsamp_max = nmax[(size_t)t];
    tab.rf_axis = true;
    return BH_OK;
}

int bh_evaluate_sites(bh_engine *e, int memspace, void *stream, int B, int Lmax, const int32_t *nlay,
                      const double *h, const double *vp, const double *vs, const double *rho,
                      ptrdiff_t stride_l, ptrdiff_t stride_b, const int32_t *site, const double *noise,
                      double *logL, double *misfits, int32_t *err, double *ymod)
{
    if (!e) return BH_EINVAL;
    if (e->sites.nsites < 1) return fail(e, BH_EINVAL, "no site table registered (bh_sites_set)");
    if (!site) return fail(e, BH_EINVAL, "null argument");
    return evaluate(e, memspace, stream, B, Lmax, nlay, h, vp, vs, rho, stride_l, stride_b, site, noise, logL, misfits, err, ymod);
}

int bh_loglike_batch(bh_engine *e, int memspace, void *stream, int B, const double *ymod,
                     const int32_t *failflags, const double *noise, double *logL, double *misfits,
                     int32_t *err)
{
    int rc;
    if (!e) return BH_EINVAL;
    if (e->nt < 1) return fail(e, BH_EINVAL, "no targets registered (bh_targets_set)");
    if (B < 0 || !ymod || !noise || !logL || !misfits || !err) return fail(e, BH_EINVAL, "null argument");
    if (B == 0) return BH_OK;
    HIPCHK(e, hipSetDevice(e->device));
    const int nt = e->nt, ldy = e->ldy;
    const bool host = (memspace != BH_DEVICE);
    hipStream_t st = (!host && stream) ? (hipStream_t)stream : e->stream;
    if ((rc = ensure(e, e->err_t, (size_t)nt * B * sizeof(int32_t)))) return rc;
    e->err_t_nt = e->err_t_B = -1; // (this call may fill the flag rows with the caller's: bh_evaluate_batch zeroes them again)
    LikeKernelArgs la{};
    la.B = B; la.nt = nt; la.ldy = ldy;
    la.ymod = ymod; la.noise = noise; la.logL = logL; la.misfits = misfits; la.err = err;
    la.err_t = failflags;
    if (host) {
        if ((rc = ensure(e, e->ymod, (size_t)B * ldy * sizeof(double)))) return rc;
        HIPCHK(e, hipMemcpyAsync(e->ymod.p, ymod, (size_t)B * ldy * sizeof(double), hipMemcpyHostToDevice, st));
        if ((rc = stage_like_io(e, st, la))) return rc;
        if (failflags) HIPCHK(e, hipMemcpyAsync(e->err_t.p, failflags, (size_t)nt * B * sizeof(int32_t), hipMemcpyHostToDevice, st));
        la.ymod = (const double *)e->ymod.p;
        la.err_t = failflags ? (const int32_t *)e->err_t.p : nullptr;
    }
    if (!la.err_t) {
        HIPCHK(e, hipMemsetAsync(e->err_t.p, 0, (size_t)nt * B * sizeof(int32_t), st));
        la.err_t = (const int32_t *)e->err_t.p;
    }
    call_begin(e, st);
    const bool unfused[BH_MAX_TARGETS] = {}; // (the caller's synthetics)
    if ((rc = run_like(e, st, la, unfused, SitePlan{}, nullptr))) return rc; // (LIKE_PLAIN, GAUSS_PLAIN)
    call_end(e, st);
    HIPCHK(e, hipGetLastError());
    if (!host) return BH_OK;
    if ((rc = return_like_io(e, st, la, logL, misfits, err))) return rc;
    HIPCHK(e, hipStreamSynchronize(st));
    return BH_OK;
}

int bh_probe_math(bh_engine *e, int op, int n, const double *in, double *out)
{
    if (!e || n < 0 || !in || !out || op < 0 || op > 23 || (op == 16 && (n & 1))) return BH_EINVAL;
    if (n == 0) return BH_OK;
    int rc;
    HIPCHK(e, hipSetDevice(e->device));
    const size_t nin = (op == 6 || op == 7) ? (size_t)2 * n : (size_t)n; // division probes read pairs
    if ((rc = ensure(e, e->probe_in, nin * sizeof(double)))) return rc;
    if ((rc = ensure(e, e->probe_out, (size_t)n * sizeof(double)))) return rc;
    HIPCHK(e, hipMemcpyAsync(e->probe_in.p, in, nin * sizeof(double), hipMemcpyHostToDevice, e->stream));
    if (op >= 17) bh_launch_swd_fa_probe(op, n, (const double *)e->probe_in.p, (double *)e->probe_out.p, e->stream);
    else if (op >= 11) bh_launch_rf_probe(op, n, (const double *)e->probe_in.p, (double *)e->probe_out.p, e->stream);
    else bh_launch_probe(op, n, (const double *)e->probe_in.p, (double *)e->probe_out.p, e->stream);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(out, e->probe_out.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return BH_OK;
}

int bh_probe_swd_secular(bh_engine *e, int evaluator, int ifunc, int mmax, int mtop, const float *d, const float *a, const float *b,
                         const float *rho, int n, const double *wvno, const double *omega, double *out)
{
    if (!e || !d || !a || !b || !rho || !wvno || !omega || !out || n < 0) return BH_EINVAL;
    if (evaluator < 0 || evaluator > 2 || (ifunc != 1 && ifunc != 2) || mmax < 2 || mmax > mtop) return fail(e, BH_EINVAL, "bad evaluator, wave type or layer count");
    if (evaluator == 2 ? mtop > 32 : mtop > BH_MAX_LAYERS) return fail(e, BH_EINVAL, "mtop beyond the evaluator's rows (2..32 lean, 2..100)");
    if (n == 0) return BH_OK;
    int rc;
    HIPCHK(e, hipSetDevice(e->device));
    const size_t nm = (size_t)4 * mtop, nin = nm + (size_t)2 * n;
    if ((rc = ensure(e, e->probe_in, nin * sizeof(double)))) return rc;
    if ((rc = ensure(e, e->probe_out, (size_t)n * sizeof(double)))) return rc;
    std::vector<double> host(nin); // [4][mtop] model (binary32 values widened), wvno[n], omega[n]
    for (int l = 0; l < mtop; ++l) {
        host[l] = (double)d[l];
        host[(size_t)mtop + l] = (double)a[l];
        host[(size_t)2 * mtop + l] = (double)b[l];
        host[(size_t)3 * mtop + l] = (double)rho[l];
    }
    for (int i = 0; i < n; ++i) {
        host[nm + i] = wvno[i];
        host[nm + n + i] = omega[i];
    }
    HIPCHK(e, hipMemcpyAsync(e->probe_in.p, host.data(), nin * sizeof(double), hipMemcpyHostToDevice, e->stream));
    const double *din = (const double *)e->probe_in.p;
    if (bh_launch_swd_secular_probe(evaluator, ifunc, mmax, mtop, din, n, din + nm, din + nm + n, (double *)e->probe_out.p, e->stream) != 0)
        return fail(e, BH_EINVAL, "secular probe refused");
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(e->stream)); // (before `host` goes, and before `out` is touched)
    HIPCHK(e, hipMemcpyAsync(out, e->probe_out.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return BH_OK;
}

} // extern "C"
