// bayhunter_amd/csrc/engine_eval.hip -- the calls of the engine's host side (bh_engine_impl.h) that evaluate models: the pure plans of a
// fused call (bh_plan_sites, bh_plan_ellip, plan_eval), the receiver-function and likelihood launches, the fused call itself
// (bh_evaluate_batch, bh_evaluate_sites) and, beside it, bh_rf_batch, bh_loglike_batch and the probes.  The dispersion launches of a
// fused call are engine_swd.hip's.
#include "bh_engine_impl.h"

using namespace bheng;

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

// ... under a count table whose ellipticity targets may carry their own periods (include/bh_engine_sites_ellip.h): pure as well
extern "C" int bh_plan_ellip_sites(int nt, const bh_ellip_plan_target *T, const int32_t *own, int nsites, const int32_t *n,
                                   const double *x, int ldx, const int32_t *off, int32_t *source)
{
    if (nt < 0 || nt > BH_MAX_TARGETS || nsites < 1 || ldx < 0 || !T || !own || !n || !x || !off || !source) return -1;
    int added = 0;
    for (int t = 0; t < nt; ++t) {
        source[t] = -2;
        if (T[t].kind != BH_TARGET_ELLIP) continue;
        source[t] = -1;
        for (int j = 0; j < nt && own[t] && source[t] < 0; ++j) {
            if (!(T[j].kind == BH_TARGET_SWD && T[j].iwave == BH_WAVE_RAYLEIGH && T[j].igr == BH_VEL_PHASE && T[j].mode <= 1 &&
                  T[j].flsph == 0 && T[j].n <= BH_MAX_PERIODS))
                continue;
            bool same = true; // at every site that has t: j with the same count and the same bits
            for (int s = 0; s < nsites && same; ++s) {
                const int nst = n[(size_t)s * nt + t];
                if (nst <= 0) continue;
                same = n[(size_t)s * nt + j] == nst &&
                       std::memcmp(x + (size_t)s * ldx + off[j], x + (size_t)s * ldx + off[t], (size_t)nst * sizeof(double)) == 0;
            }
            if (same) source[t] = j;
        }
        added += source[t] < 0;
    }
    return added;
}

namespace {

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
            // (periods per site on an ellipticity target, bh_targets_set_ellip_sites: what bh_plan_ellip_sites decided when the count
            // table was registered)
            for (int t = 0; t < p.nt && p.sites.x_all; ++t)
                if (e->targets[(size_t)t].ell_sites && e->sites.ell_source[t] >= 0) {
                    p.ell_source[t] = e->sites.ell_source[t];
                    --p.nswd;
                }
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
int launch_rf(bh_engine *e, hipStream_t st, const ModelBatch &m, const RfJob &j, bool beside_swd, bool gated)
{
    const int B = m.B, Lmax = m.Lmax;
    if (B == 0) return BH_OK;
    const RfAsk q{B, Lmax, j.build, j.build == RF_SITEAXIS ? j.sites.nsamp_max : j.nsamp, j.fsamp, j.gauss, beside_swd, gated, e->rf_lds_beside_swd};
    const RfPlan p = bh_plan_rf(q, bh_tuning());
    if (p.code != BH_OK) return fail(e, p.code, bh_rf_refusal_text(p.refusal));
    if (int rc = ensure(e, e->coef, (size_t)B * bh_rf_coef_doubles(Lmax) * sizeof(double))) return rc;
    if (int rc = p.workspace ? ensure(e, e->rfz, p.work_bytes) : BH_OK) return rc;
    RfKernelArgs a{}; // (lds_min and coef_small stay 0: unused)
    a.B = B; a.Lmax = Lmax; a.nsamp = j.nsamp; a.nkeep = j.nkeep; a.waveno = j.waveno;
    a.nlay = m.nlay; a.h = m.h; a.vp = m.vp; a.vs = m.vs; a.rho = m.rho; a.qp = m.qp; a.qs = m.qs; a.sl = m.sl; a.sb = m.sb;
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

} // namespace

namespace bheng {

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

} // namespace bheng

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
    ModelBatch m;
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

__global__ void rho_from_vp_kernel(size_t n, const double *vp, double *rho)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) rho[i] = vp[i] * 0.32 + 0.77; // Targets.py:319
}

// A BH_HOST call's arrays go to the engine's staging buffers; the density where the caller gave none
int stage_eval_inputs(bh_engine *e, bool host, EvalCall &c)
{
    const int B = c.m.B;
    int rc;
    if (host) {
        if ((rc = stage_models(e, c.m))) return rc;
        if ((rc = stage_like_io(e, c.st, c.la))) return rc;
        if (c.site) {
            if ((rc = ensure(e, e->sites.idx, (size_t)B * sizeof(int32_t)))) return rc;
            HIPCHK(e, hipMemcpyAsync(e->sites.idx.p, c.site, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, c.st));
            c.site = (const int32_t *)e->sites.idx.p;
        }
        c.ymod = nullptr;
    }
    if (!c.m.rho) { // rho = 0.32 vp + 0.77 (Targets.py:319)
        const size_t nel = span_elems(c.m);
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
    // every site shares -- or, bh_targets_set_ellip_sites, every site's own periods and count, the job's K being the capacity.)
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
    const SwdPlan swp = plan_swd_call(e, c.m, njobs, jobs);
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
    if ((rc = launch_swd_jobs(e, st, c.m, njobs, jobs, swp, fills, p.prio_low, &swd))) return rc;
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
        if ((rc = launch_rf(e, rst, c.m, job, p.fork, gate))) return rc;
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
        a.B = B; a.Lmax = c.m.Lmax; a.K = T.d.n; a.nsteps = T.ell_nsteps; a.is_signed = T.ell_signed; a.zh = T.ell_zh;
        a.nlay = c.m.nlay; a.h = c.m.h; a.vp = c.m.vp; a.vs = c.m.vs; a.rho = c.m.rho;
        a.sl = c.m.sl; a.sb = c.m.sb;
        a.periods = (const double *)T.x.p;
        a.vel = j >= 0 ? c.ymod + e->targets[(size_t)j].off : (const double *)T.ell_vel.p;
        a.ldvel = j >= 0 ? ldy : T.d.n;
        a.y = c.ymod + T.off; a.ldy = ldy;
        a.err_row = row;
        if (T.ell_sites) { // (K: the capacity; a lane's period and its model's count are the table's, column t)
            a.site = c.site; a.nsites = S.nsites;
            a.xn = (const int32_t *)S.xn.p + t; a.ldn = nt;
            a.xper = (const double *)S.xper.p + T.off; a.ldx = ldy;
        }
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
    const ModelBatch m{B, Lmax, nlay, h, vp, vs, rho, nullptr, nullptr, sl, sb};
    if ((rc = check_models(e, m))) return rc;
    if (!site) // (bh_evaluate_batch reads no table: include/bh_engine_sites_ellip.h)
        for (const TargetHost &T : e->targets)
            if (T.ell_sites) return fail(e, BH_EINVAL, "bh_evaluate_batch: an ellipticity target with periods per site (bh_targets_set_ellip_sites) is served by bh_evaluate_sites");
    const bool host = (memspace != BH_DEVICE);
    const EvalPlan p = plan_eval(e, B, site != nullptr, ymod != nullptr);
    LikeKernelArgs la{};
    la.B = B; la.nt = p.nt; la.ldy = p.ldy; la.noise = noise; la.logL = logL; la.misfits = misfits; la.err = err;
    EvalCall c{(!host && stream) ? (hipStream_t)stream : e->stream, m, site, ymod, la};
    if ((rc = eval_args_ok(e, p, host, c))) return rc;
    if (B == 0) return BH_OK;
    HIPCHK(e, hipSetDevice(e->device));
    if ((rc = stage_eval_inputs(e, host, c)) || (rc = size_eval_workspaces(e, p, c))) return rc;
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

int bh_rf_batch(bh_engine *e, int memspace, void *stream, int B, int Lmax, const int32_t *nlay,
                const double *h, const double *vp, const double *vs, const double *rho,
                const double *qp, const double *qs, ptrdiff_t sl, ptrdiff_t sb, double p,
                double gauss, int nsamp, double fsamp, double tshift, double nsv, int waveno,
                int nkeep, double *rf)
{
    int rc;
    ModelBatch m{B, Lmax, nlay, h, vp, vs, rho, qp, qs, sl, sb};
    if ((rc = check_models(e, m))) return rc;
    if ((rc = rf_args_ok(e, nsamp, nkeep, gauss, fsamp, waveno))) return rc;
    if (!nlay || !h || !vp || !vs || !rho || !rf) return fail(e, BH_EINVAL, "null argument");
    if (B == 0 || nkeep == 0) return BH_OK;
    HIPCHK(e, hipSetDevice(e->device));
    const bool host = (memspace != BH_DEVICE);
    hipStream_t st = (!host && stream) ? (hipStream_t)stream : e->stream;
    RfJob job{p, gauss, nsamp, fsamp, tshift, nsv, waveno, nkeep, rf, nkeep, nullptr, nullptr, RF_PLAIN, RfSiteTArgs{}};
    if (host) {
        if ((rc = stage_models(e, m))) return rc;
        if ((rc = ensure(e, e->rf, (size_t)B * nkeep * sizeof(double)))) return rc;
        job.rf = (double *)e->rf.p;
    }
    call_begin(e, st);
    rc = launch_rf(e, st, m, job, false, false); // (not beside anything)
    call_end(e, st);
    if (rc || !host) return rc;
    HIPCHK(e, hipMemcpyAsync(rf, e->rf.p, (size_t)B * nkeep * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    return BH_OK;
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
