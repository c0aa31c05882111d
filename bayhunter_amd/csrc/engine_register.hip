// bayhunter_amd/csrc/engine_register.hip -- what the engine's host side (bh_engine_impl.h) registers once and the calls then read: the
// targets (bh_targets_set, bh_targets_set_ellip) and every part of the site table (bh_sites_set*).  Checks on the host, then uploads
// (upload, one step each); no launch, no per-call path.
#include "bh_engine_impl.h"

using namespace bheng;

extern "C" {

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
        if (!rc) rc = upload(e, t.yobs, d.yobs, nb, "upload yobs");
        if (!rc && d.kind == BH_TARGET_SWD) {
            rc = upload(e, t.x, d.x, nb, "upload x");
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
                rc = upload(e, t.x60, g, sizeof(g), "upload x60");
            }
        }
        if (!rc && d.law == BH_LAW_NOCORR_SCALED) { // Targets.py:124-128
            std::vector<double> se((size_t)d.n);
            t.logdet_extra = scaled_errors(d.yerr, d.n, se.data());
            rc = upload(e, t.yerr_scaled, se.data(), nb, "upload yerr");
        }
        if (!rc && d.law == BH_LAW_GAUSS) {
            t.logdet_extra = d.logdet_r;
            rc = upload(e, t.rinv, d.rinv, nb * (size_t)d.n, "upload rinv");
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
    if (int rc = upload(e, T.x, periods, (size_t)K * sizeof(double), "upload ellipticity periods")) return rc;
    T.x_host.assign(periods, periods + K);
    T.xid = period_id(e->targets, t, e->nt);
    T.ell_nsteps = nsteps; T.ell_signed = is_signed != 0; T.ell_zh = zh != 0;
    T.d.kind = BH_TARGET_ELLIP;
    T.d.iwave = BH_WAVE_RAYLEIGH; T.d.igr = BH_VEL_PHASE; T.d.mode = 1; T.d.flsph = 0; // (what its own search runs)
    T.kfwd = K;
    e->err_t_nt = e->err_t_B = -1;
    return BH_OK;
}

int bh_targets_set_ellip_sites(bh_engine *e, int t, int own)
{
    if (!e) return BH_EINVAL;
    if (t < 0 || t >= e->nt) return fail(e, BH_EINVAL, "bh_targets_set_ellip_sites: no such target (bh_targets_set)");
    if (e->targets[(size_t)t].d.kind != BH_TARGET_ELLIP) return fail(e, BH_EINVAL, "bh_targets_set_ellip_sites: the target is not a BH_TARGET_ELLIP (bh_targets_set_ellip)");
    if (e->sites.nsites > 0) return fail(e, BH_EINVAL, "bh_targets_set_ellip_sites: a site table is in force (call it between bh_targets_set_ellip and bh_sites_set*)");
    e->targets[(size_t)t].ell_sites = own != 0;
    return BH_OK;
}

// the first registered ellipticity target with periods per site (bh_targets_set_ellip_sites), or -1
static int first_ellip_sites(const bh_engine *e)
{
    for (int t = 0; t < e->nt; ++t)
        if (e->targets[(size_t)t].d.kind == BH_TARGET_ELLIP && e->targets[(size_t)t].ell_sites) return t;
    return -1;
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
    if ((rc = upload(e, tab.yobs, n ? yo.data() : yobs, S * ldy * sizeof(double), "upload site table")) ||
        (rc = upload(e, tab.yerr, se.data(), S * ldy * sizeof(double), "upload site table")) ||
        (rc = upload(e, tab.logdet, ld.data(), S * nt * sizeof(double), "upload site table"))) {
        tab.drop(PART_COUNTS);
        return rc;
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
    if (first_ellip_sites(e) >= 0)
        return fail(e, BH_EINVAL, "bh_sites_set: an ellipticity target with periods per site (bh_targets_set_ellip_sites) needs the table of bh_sites_set_x_all or of a later entry point");
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
    if (!admits_any_dispersion && first_ellip_sites(e) >= 0)
        return fail(e, BH_EINVAL, (w + ": an ellipticity target with periods per site (bh_targets_set_ellip_sites) needs the table of bh_sites_set_x_all or of a later entry point").c_str());
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
        // (an ellipticity target with periods per site, bh_targets_set_ellip_sites: the rules of a dispersion curve, below)
        if (d.kind != BH_TARGET_SWD && !(d.kind == BH_TARGET_ELLIP && T.ell_sites)) { // (a receiver function's x is its descriptor's time axis: shared, but for bh_sites_set_axes)
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
            for (size_t s = 0; s < S; ++s) // (x_host: the bits bh_targets_set uploaded)
                if (n[s * nt + t] != d.n || std::memcmp(T.x_host.data(), x + s * ldy + T.off, (size_t)d.n * sizeof(double)) != 0)
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
    if ((rc = upload(e, tab.xn, n, S * nt * sizeof(int32_t), "upload site table")) ||
        (rc = upload(e, tab.xper, xs.data(), S * ldy * sizeof(double), "upload site table"))) {
        tab.drop(PART_COUNTS);
        return rc;
    }
    tab.level = level;
    tab.xn_host.assign(n, n + S * nt);
    if (first_ellip_sites(e) >= 0) { // where the ellipticity targets with periods per site take their velocities: decided once, here
        bh_ellip_plan_target q[BH_MAX_TARGETS];
        int32_t own[BH_MAX_TARGETS], off[BH_MAX_TARGETS];
        for (int t = 0; t < nt; ++t) {
            const TargetHost &T = e->targets[(size_t)t];
            q[t] = bh_ellip_plan_target{T.d.kind, T.d.iwave, T.d.igr, T.d.mode, T.d.flsph, T.d.n, T.xid};
            own[t] = T.ell_sites ? 1 : 0;
            off[t] = T.off;
        }
        (void)bh_plan_ellip_sites(nt, q, own, nsites, n, xs.data(), ldy, off, tab.ell_source);
    }
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
    if ((rc = upload(e, G.rinv, rinv, (size_t)nclass * nn * sizeof(double), "upload class matrices")) ||
        (rc = upload(e, G.logdet, logdet_r, (size_t)nclass * sizeof(double), "upload class matrices")) ||
        (rc = upload(e, G.class_of, class_of, S * sizeof(int32_t), "upload class matrices")))
        return rc;
    if (tab.level < SITES_X && !tab.desc_n.p) { // no count table in force: the likelihood build of the class calls reads the descriptors' counts
        std::vector<int32_t> cnt(S * nt);
        for (size_t s = 0; s < S; ++s)
            for (size_t t = 0; t < nt; ++t) cnt[s * nt + t] = e->targets[t].d.n;
        if ((rc = upload(e, tab.desc_n, cnt.data(), S * nt * sizeof(int32_t), "upload descriptor counts"))) return rc;
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
    if ((rc = upload(e, tab.law, lw.data(), S * nt * sizeof(int32_t), "upload law table")) ||
        (rc = upload(e, tab.law_yerr, se.data(), S * ldy * sizeof(double), "upload law table")) ||
        (rc = upload(e, tab.law_logdet, ld.data(), S * nt * sizeof(double), "upload law table")))
        return rc;
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
    if ((rc = upload(e, tab.p, p_s_per_deg, n * sizeof(double), "upload receiver-function table")) ||
        (rc = upload(e, tab.nsv, nsv, n * sizeof(double), "upload receiver-function table")))
        return rc;
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
    if (int rc = upload(e, tab.axis, recs.data(), recs.size() * sizeof(RfAxisRec), "upload axis table")) return rc;
    for (int t = 0; t < nt; ++t) tab.t[t].axis_nsamp_max = nmax[(size_t)t];
    tab.rf_axis = true;
    return BH_OK;
}

} // extern "C"
