"""Dispersion periods per site on the MI355X (include/bh_engine_sites_x.h, SiteTargets(per_site_x=True)): bh_evaluate_sites with
each site's own periods against each site's own bh_evaluate_batch, bit for bit, on the site-period builds of the trial-per-lane
and group kernels and of the likelihood kernels; against the oracle; independence of the batch's order and composition; the
API's refusals and lifetime; DeviceChains over sites of different period counts against one-site runs."""
import pickle

import numpy as np
import pytest

from conftest import golden
import bayhunter_amd as bh
from bayhunter_amd import engine as E
from bayhunter_amd.device_chains import DeviceChains
from bayhunter_amd.synth import synth_models, prior_models
from test_gpu_sites import eval_device

pytestmark = pytest.mark.gpu

# Six sites: 30 periods; every second of them (surfdisp96 starts period k from the root at period k - 1: not the same curve);
# seven unevenly spaced short periods; a single period; 60 periods (the most a site may have); and site 0's periods again
# with other observed data.
X30 = np.linspace(2, 60, 30)
PERIOD_SETS = [X30, X30[::2].copy(), np.array([1.0, 1.7, 2.9, 4.0, 6.5, 8.1, 11.0]), np.array([20.0]), np.geomspace(1, 40, 60), X30.copy()]
NSITES = len(PERIOD_SETS)
SITE_P = np.array([5.0, 5.5, 6.4, 7.0, 7.5, 8.0])       # with per_site_rf: each site's ray parameter (s/deg)
B_MODELS = 660                                          # 110 models per site
FAMILIES = ("synth", "prior")
LMAX = (8, 21, 40)
LAWS_OF = {"nocorr_exp": (E.LAW_NOCORR, E.LAW_EXP), "scaled": (E.LAW_NOCORR_SCALED, E.LAW_NOCORR_SCALED),
           "joint": (E.LAW_NOCORR_SCALED, E.LAW_EXP)}


def batch(family, Lmax):
    """(nlay, h, vp, vs, rho, site) of the fixed batch of a (family, array capacity): ragged sorted-velocity models or models
    drawn from a sampler's prior (arrays of 8 layers: at least 4, so that Love fails on fewer than 30 % of them at every
    period set -- tests/test_sites_x_host.py asserts the shares with the oracle), every site 110 models in random places."""
    rs = np.random.RandomState(1000 + Lmax + (7 if family == "prior" else 0))
    if family == "synth":
        mods = synth_models(rs, B_MODELS, Lmax, ragged=True)
    else:
        mods = prior_models(rs, B_MODELS, Lmax, nmin=4 if Lmax == 8 else 2)
    site = (rs.permutation(B_MODELS) % NSITES).astype(np.int32)
    return mods + (site,)


def site_descs(case, rs, period_sets=PERIOD_SETS):
    """every site's own one-site descriptors: Rayleigh and Love phase velocities at its periods (laws of the case, yerr per
    site) and, case "joint", a P receiver function with its own ray parameter"""
    out = []
    for s, per in enumerate(period_sets):
        n, ds = per.size, []
        for iwave, law in zip((2, 1), LAWS_OF[case]):
            d = dict(kind=E.TARGET_SWD, law=law, n=n, x=per, iwave=iwave, igr=0, yobs=3.0 + 0.3 * np.log(per) + rs.normal(0, 0.05, n))
            if law == E.LAW_NOCORR_SCALED:
                d["yerr"] = rs.uniform(0.01, 0.05, n)
            ds.append(d)
        if case == "joint":
            ds.append(dict(kind=E.TARGET_RF, law=E.LAW_EXP, n=150, waveno=0, nsamp=512, p=float(SITE_P[s]), gauss=2.5, fsamp=5.0,
                           tshift=5.0, nsv=0.0, yobs=rs.normal(0, 0.05, 150)))
        out.append(ds)
    return out


def tables(descs):
    """capacity descriptors (site 0's with every dispersion target's n the largest of any site and placeholders for x, yobs,
    yerr) and the tables n[S, nt], x, yobs, yerr[S, ldy] of bh_sites_set_x, p, nsv[S, nt] of bh_sites_set_rf"""
    S, nt = len(descs), len(descs[0])
    n = np.array([[d["n"] for d in ds] for ds in descs], dtype=np.int32)
    cap = n.max(axis=0)
    off = np.concatenate([[0], np.cumsum(cap)]).astype(int)
    x, yobs, yerr = np.zeros((S, off[-1])), np.zeros((S, off[-1])), np.ones((S, off[-1]))
    for s, ds in enumerate(descs):
        for t, d in enumerate(ds):
            c = slice(off[t], off[t] + d["n"])
            yobs[s, c] = d["yobs"]
            if d["kind"] == E.TARGET_SWD:
                x[s, c] = d["x"]
            if "yerr" in d:
                yerr[s, c] = d["yerr"]
    caps = []
    for t, d in enumerate(descs[0]):
        d = dict(d)
        if d["kind"] == E.TARGET_SWD:
            d.update(n=int(cap[t]), x=np.ones(cap[t]), yobs=np.zeros(cap[t]))
            if "yerr" in d:
                d["yerr"] = np.ones(cap[t])
        caps.append(d)
    scaled = any("yerr" in d for d in descs[0])
    p = np.array([[d.get("p", 0.0) for d in ds] for ds in descs])
    return caps, n, x, yobs, (yerr if scaled else None), p, np.zeros_like(p), off


def register(eng, descs):
    caps, n, x, yobs, yerr, p, nsv, off = tables(descs)
    eng.set_targets(caps)
    eng.set_sites_x(n, x, yobs, yerr)
    if any(d["kind"] == E.TARGET_RF for d in descs[0]):
        eng.set_sites_rf(p, nsv)
    return n, off


def padded(ymod, ns, off):
    """a one-site ymod [B, sum n] in the columns of the site table's layout: every target's n values, zeros up to its capacity"""
    out = np.zeros((ymod.shape[0], off[-1]))
    o = 0
    for t, k in enumerate(ns):
        out[:, off[t]:off[t] + k] = ymod[:, o:o + k]
        o += k
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def assert_site_bits(got, ref, m, ns, off, what):
    """logL, misfits, err and the WHOLE ymod row (failed models and the zero padding included) of the models m, bit for bit"""
    ref = (ref[0], ref[1], ref[2], padded(ref[3], ns, off))
    for k, (a, b) in enumerate(zip(got, ref)):
        assert np.array_equal(bits(a[m]), bits(b[m])), "%s: %s" % (what, ("logL", "misfits", "err", "ymod")[k])


SETTINGS = [("default", 4), ("default", 16), ("default", 32), ("default", 64), ("reference", 0), ("exact", 0)]


def configure(eng, setting, trials):
    eng.set_swd_search("reference" if setting == "reference" else "fast")
    eng.set_swd_arith("exact" if setting == "exact" else "fast")
    eng.set_swd_trials(trials)


def lean_fits(trials, Lmax, kmax, per_model):
    """the trial-per-lane kernel's LDS request (swd_lean.hip: lean_wave_lds) within the 64 KB of a workgroup"""
    mpw = 64 // trials
    return Lmax <= 32 and 4 * (((((kmax + 1) & ~1) * (mpw if per_model else 1) + 7 * Lmax * mpw) * 8 + 15) & ~15) <= 64 * 1024


@pytest.mark.parametrize("Lmax", LMAX)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", ["nocorr_exp", "scaled", "joint"])
def test_per_site_x_equals_each_sites_own_evaluation(engine, case, family, Lmax):
    rs = np.random.RandomState(Lmax + 13 * len(case) + len(family))
    descs = site_descs(case, rs)
    nt = len(descs[0])
    nlay, h, vp, vs, rho, site = batch(family, Lmax)
    mods = (nlay, h, vp, vs, rho)
    noise = np.column_stack([rs.uniform(0.1, 0.6, B_MODELS) if i % 2 == 0 else rs.uniform(0.02, 0.1, B_MODELS) for i in range(2 * nt)])
    for t, d in enumerate(descs[0]):
        if d["law"] != E.LAW_EXP:
            noise[:, 2 * t] = 0.0
    assert min(np.bincount(site, minlength=NSITES)) >= 100
    try:
        for setting, trials in SETTINGS:
            what = "%s %s Lmax %d, %s %d" % (case, family, Lmax, setting, trials)
            configure(engine, setting, trials)
            refs, ref_kernel = [], []
            for ds in descs:     # every site alone: the same models, that site's descriptors, the same pinned trial count
                engine.set_targets(ds)
                refs.append(engine.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True))
                ref_kernel.append(engine.last_swd_kernel())
            n, off = register(engine, descs)
            got = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
            kernel, launches = engine.last_swd_kernel(), engine.last_swd_launches()
            guarded = sum(engine.guard_stats()[0])
            dev = eval_device(engine, mods, noise, site, engine.ldy)
            assert engine.ldy == off[-1] and got[3].shape == (B_MODELS, off[-1])
            covered = np.zeros(B_MODELS, bool)
            for s in range(NSITES):
                m = site == s
                covered |= m
                assert_site_bits(got, refs[s], m, n[s], off, "%s, site %d host" % (what, s))
                assert_site_bits(dev, refs[s], m, n[s], off, "%s, site %d device" % (what, s))
                for t in range(2):          # beyond a site's own periods: zeros up to the capacity
                    assert np.all(got[3][m, off[t] + n[s, t]:off[t + 1]] == 0.0)
            assert covered.all()            # no model is left out of the comparison
            roles = {(l["family"], l["role"]) for l in launches}
            if setting == "default":
                # the bits depend on the kernel family and the trial count: both sides took the same one
                want = "lean" if lean_fits(trials, Lmax, 60, True) else "group"
                assert kernel == want and all(k == want for k in ref_kernel), (what, kernel, ref_kernel)
                assert (want, "main") in roles, (what, roles)
                if want == "lean":          # the models its guard lists: the group kernel's re-run, site periods carried along
                    assert ("group", "rerun") in roles, (what, roles)
                if family == "prior" and trials == 16 and want == "lean":
                    assert guarded > 0, what        # ... and it has models to run
            else:                           # every kernel returns the same bits; the sites side has no one-lane-per-evaluation build
                assert kernel in ("lean", "group"), (what, kernel)
            if setting == "default" and trials == 16:
                ok = got[2] == 0
                assert ok.sum() > 0.5 * B_MODELS
                assert np.isfinite(got[0][ok]).all()
    finally:
        engine.set_swd_trials(0)


def test_every_launch_kind_of_the_site_period_builds_occurs(engine):
    """"lean" main, "group" main and "group" re-run launches of a sites call with a period table (the parametrisation above
    asserts them case by case; here in one place, on one small batch each)"""
    rs = np.random.RandomState(5)
    descs = site_descs("nocorr_exp", rs)
    seen = set()
    try:
        for Lmax, setting in ((8, "default"), (40, "default"), (21, "reference")):
            nlay, h, vp, vs, rho, site = batch("prior", Lmax)
            noise = np.tile([0.0, 0.05, 0.4, 0.05], (B_MODELS, 1))
            configure(engine, setting, 16 if setting == "default" else 0)
            register(engine, descs)
            engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho)
            seen |= {(l["family"], l["role"]) for l in engine.last_swd_launches()}
    finally:
        engine.set_swd_trials(0)
    assert {("lean", "main"), ("group", "main"), ("group", "rerun")} <= seen, seen
    assert not [k for k in seen if k[0] == "lane"], seen


@pytest.mark.parametrize("Lmax", [8, 21])
@pytest.mark.parametrize("family", FAMILIES)
def test_per_site_x_against_the_oracle(engine, oracle, family, Lmax):
    """Velocities and flags of every site against oracle.swd_batch with that site's periods: bit-identical with
    search="reference"; with the defaults flags and zero rows identical and velocities within the bound the default path is
    held to on these model families (tests/test_gpu_swd_lean.py 2e-6, tests/test_gpu_fuzz.py 2.5e-6 on prior-like models).
    logL against oracle.loglike_dense on the device's own synthetics: 1e-8."""
    rs = np.random.RandomState(40 + Lmax)
    descs = site_descs("joint", rs)
    nlay, h, vp, vs, rho, site = batch(family, Lmax)
    noise = np.column_stack([np.zeros(B_MODELS), rs.uniform(0.02, 0.1, B_MODELS), rs.uniform(0.2, 0.8, B_MODELS),
                             rs.uniform(0.02, 0.1, B_MODELS), rs.uniform(0.2, 0.8, B_MODELS), rs.uniform(0.02, 0.1, B_MODELS)])
    want = {}
    for s, per in enumerate(PERIOD_SETS):
        m = site == s
        for t, iwave in enumerate((2, 1)):
            v, e, _ = oracle.swd_batch(nlay[m], h.T[m], vp.T[m], vs.T[m], rho.T[m], per, iwave, 0)
            assert (e != 0).mean() <= 0.30, (family, Lmax, s, iwave, (e != 0).mean())     # the test is not about zero rows
            want[s, t] = (v, e)
    bound = 2.5e-6 if family == "prior" else 2e-6
    try:
        for setting, trials in (("reference", 0), ("default", 0), ("default", 16)):
            configure(engine, setting, trials)
            n, off = register(engine, descs)
            logL, misf, err, ymod = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
            for s, per in enumerate(PERIOD_SETS):
                m = site == s
                bad = np.zeros(m.sum(), bool)
                for t in range(2):
                    v, e = want[s, t]
                    got = ymod[m, off[t]:off[t] + per.size]
                    bad |= e != 0
                    if setting == "reference":
                        assert np.array_equal(bits(got), bits(v)), (family, Lmax, s, t)
                    else:
                        assert np.array_equal(got == 0, v == 0), (family, Lmax, s, t, trials)
                        both = v != 0
                        worst = np.max(np.abs(got[both] - v[both]) / np.abs(v[both]))
                        assert worst <= bound, (family, Lmax, s, t, trials, worst)
                assert np.array_equal(err[m] != 0, bad), (family, Lmax, s, setting)
                assert np.all(logL[m][bad] == -1e15)
                for b in np.flatnonzero(m)[~bad][:12]:      # the likelihood as a function of the device's own synthetics
                    ds, o = descs[s], 0.0
                    for t, d in enumerate(ds):
                        y = ymod[b, off[t]:off[t] + d["n"]]
                        o += oracle.loglike_dense(d["law"], y, d["yobs"], noise[b, 2 * t], noise[b, 2 * t + 1], yerr=d.get("yerr"))
                    assert abs(logL[b] - o) <= 1e-8 * abs(o), (family, Lmax, s, b, logL[b], o)
    finally:
        engine.set_swd_trials(0)


@pytest.mark.parametrize("setting,trials,Lmax", [("default", 16, 21), ("default", 32, 8), ("default", 0, 40), ("reference", 0, 21)])
def test_results_do_not_depend_on_order_numbering_or_company(engine, setting, trials, Lmax):
    rs = np.random.RandomState(17 + Lmax)
    descs = site_descs("joint", rs)
    nlay, h, vp, vs, rho, site = batch("prior", Lmax)
    nt = 3
    noise = np.column_stack([rs.uniform(0.1, 0.6, B_MODELS) if i % 2 == 0 else rs.uniform(0.02, 0.1, B_MODELS) for i in range(2 * nt)])
    noise[:, 0] = 0.0
    try:
        configure(engine, setting, trials)
        register(engine, descs)
        base = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
        # the batch permuted
        q = rs.permutation(B_MODELS)
        got = engine.evaluate_sites(nlay[q], h[:, q], vp[:, q], vs[:, q], noise[q], site[q], rho=rho[:, q], want_ymod=True)
        for a, b in zip(got, base):
            assert np.array_equal(bits(a), bits(b[q])), "permuted"
        # the sites renumbered
        r = rs.permutation(NSITES)                       # new number of site s: r[s]
        inv = np.argsort(r)
        register(engine, [descs[inv[k]] for k in range(NSITES)])
        got = engine.evaluate_sites(nlay, h, vp, vs, noise, r[site].astype(np.int32), rho=rho, want_ymod=True)
        for a, b in zip(got, base):
            assert np.array_equal(bits(a), bits(b)), "renumbered"
        # one site's models alone in the call (the trial count is pinned; the group kernel's plan is the batch's shape: the
        # reference's sequence returns the same bits from every plan, the defaults are compared at the pinned trial counts)
        if not (setting == "default" and trials == 0):
            register(engine, descs)
            for s in (1, 3, 4):
                m = site == s
                got = engine.evaluate_sites(nlay[m], h[:, m], vp[:, m], vs[:, m], noise[m], site[m], rho=rho[:, m], want_ymod=True)
                for a, b in zip(got, base):
                    assert np.array_equal(bits(a), bits(b[m])), "site %d alone" % s
        # every site with the same x: the existing shared-x sites path
        same = site_descs("joint", np.random.RandomState(3), period_sets=[X30] * NSITES)
        caps, n, x, yobs, yerr, p, nsv, off = tables(same)
        engine.set_targets(same[0])
        engine.set_sites(yobs, yerr)
        engine.set_sites_rf(p, nsv)
        shared = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
        shared_kernel = engine.last_swd_kernel()
        register(engine, same)
        got = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
        if setting == "default":
            assert engine.last_swd_kernel() == shared_kernel
        for a, b in zip(got, shared):
            assert np.array_equal(bits(a), bits(b)), "shared x"
    finally:
        engine.set_swd_trials(0)


def test_api_refusals_and_lifetime(engine):
    rs = np.random.RandomState(4)
    descs = site_descs("joint", rs)
    nlay, h, vp, vs, rho, site = batch("synth", 8)
    B = 120
    nlay, h, vp, vs, rho, site = nlay[:B], h[:, :B], vp[:, :B], vs[:, :B], rho[:, :B], site[:B]
    noise = np.tile([0.0, 0.05, 0.4, 0.05, 0.5, 0.03], (B, 1))
    caps, n, x, yobs, yerr, p, nsv, off = tables(descs)
    L, hd = engine._L, engine._h
    P = lambda a: a.ctypes.data
    S = NSITES

    def rc(n_=n, x_=x, yobs_=yobs, yerr_=yerr, S_=S):
        return L.bh_sites_set_x(hd, S_, P(n_) if n_ is not None else None, P(x_) if x_ is not None else None,
                                P(yobs_) if yobs_ is not None else None, P(yerr_) if yerr_ is not None else None)

    engine.set_targets(caps)
    batch0 = engine.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True)
    # null arguments, a count below 1 or above the capacity, periods that are not finite and positive, an RF count
    assert rc(n_=None) == E.BH_EINVAL and rc(x_=None) == E.BH_EINVAL and rc(yobs_=None) == E.BH_EINVAL
    assert rc(yerr_=None) == E.BH_EINVAL            # a scaled-error target needs yerr
    assert rc(S_=0) == E.BH_EINVAL
    for bad in (0, -3, 61):
        b = n.copy()
        b[2, 1] = bad
        assert rc(n_=b) == E.BH_EINVAL, bad
    b = n.copy()
    b[1, 2] -= 1                                    # a receiver function's count is its descriptor's
    assert rc(n_=b) == E.BH_EINVAL
    for bad in (0.0, -2.0, np.nan, np.inf):
        b = x.copy()
        b[1, off[1] + 3] = bad
        assert rc(x_=b) == E.BH_EINVAL, bad
    b = x.copy()
    b[1, off[1] + n[1, 1]] = np.nan                 # beyond a site's own count nothing is read
    assert rc(x_=b) == E.BH_OK
    engine.set_targets(caps)
    assert rc(x_=None) == E.BH_EINVAL
    with pytest.raises(E.EngineError, match="site table"):      # nothing is registered by a refused call
        engine.set_sites_rf(p, nsv)
    # the Gauss law on a dispersion target; group velocities, higher modes and more than 60 periods with periods per site
    g = [dict(d) for d in caps]
    g[1].update(law=E.LAW_GAUSS, rinv=np.eye(g[1]["n"]), logdet_r=0.0)
    engine.set_targets(g)
    assert rc() == E.BH_EINVAL
    for change in (dict(igr=1), dict(mode=2)):
        g = [dict(d) for d in caps]
        g[0].update(change)
        engine.set_targets(g)
        assert rc() == E.BH_EUNSUPPORTED, change
    same = tables(site_descs("joint", np.random.RandomState(3), period_sets=[X30] * NSITES))
    g = [dict(d) for d in same[0]]
    g[0].update(igr=1, x=X30)                       # ... but fine where every site has the descriptor's periods
    engine.set_targets(g)
    assert L.bh_sites_set_x(hd, S, P(same[1]), P(same[2]), P(same[3]), P(same[4])) == E.BH_OK
    b = same[2].copy()
    b[3, 7] = np.nextafter(b[3, 7], 100.0)
    assert L.bh_sites_set_x(hd, S, P(same[1]), P(b), P(same[3]), P(same[4])) == E.BH_EUNSUPPORTED
    big = [dict(kind=E.TARGET_SWD, law=E.LAW_NOCORR, n=61, x=np.linspace(2, 60, 61), iwave=2, igr=0, yobs=np.zeros(61))]
    engine.set_targets(big)
    assert L.bh_sites_set_x(hd, 1, P(np.array([[61]], np.int32)), P(np.linspace(2, 60, 61)[None].copy()), P(np.zeros((1, 61))), None) == E.BH_EUNSUPPORTED
    # lifetime: bh_sites_set and bh_targets_set drop the table
    engine.set_targets(caps)
    engine.set_sites_x(n, x, yobs, yerr)
    engine.set_sites_rf(p, nsv)
    own = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
    engine.set_sites(yobs, yerr)                    # the plain table: the descriptors' placeholder periods (1 s) at every site
    plain = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
    assert not np.array_equal(plain[3][:, :off[2]], own[3][:, :off[2]]) and np.all(plain[3][plain[2] == 0, :off[2]] != 0.0)
    engine.set_sites_x(n, x, yobs, yerr)
    engine.set_sites_rf(p, nsv)
    again = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
    for a, b in zip(again, own):
        assert np.array_equal(bits(a), bits(b))
    engine.set_targets(caps)
    with pytest.raises(E.EngineError, match="site table"):
        engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho)
    # a device-side site out of range fails in band and reads nothing; the others are untouched
    engine.set_sites_x(n, x, yobs, yerr)
    engine.set_sites_rf(p, nsv)
    wild = site.copy()
    wild[5], wild[17] = NSITES, -1
    dev = eval_device(engine, (nlay, h, vp, vs, rho), noise, wild, engine.ldy)
    for b in (5, 17):
        assert dev[2][b] == 1 and dev[0][b] == -1e15 and np.all(dev[1][b] == 1e15) and np.all(dev[3][b, :off[2]] == 0.0)
    keep = np.ones(B, bool)
    keep[[5, 17]] = False
    for a, b in zip(dev, own):
        assert np.array_equal(bits(a[keep]), bits(b[keep]))
    with pytest.raises(E.EngineError, match="out of range"):    # host memspace: checked before anything is launched
        engine.evaluate_sites(nlay, h, vp, vs, noise, wild, rho=rho)
    # ... the same on the group kernel's site-period builds (the reference's sequence; arrays of 40 layers with the defaults)
    for Lmax, setting in ((21, "reference"), (40, "default")):
        gl, gh, gvp, gvs, grho, gsite = [a[..., :B] for a in batch("prior", Lmax)]
        configure(engine, setting, 0)
        good = eval_device(engine, (gl, gh, gvp, gvs, grho), noise, gsite, engine.ldy)
        assert engine.last_swd_kernel() == "group"
        wild = gsite.copy()
        wild[5], wild[17] = NSITES, -1
        dev = eval_device(engine, (gl, gh, gvp, gvs, grho), noise, wild, engine.ldy)
        assert engine.last_swd_kernel() == "group"
        for b in (5, 17):
            assert dev[2][b] == 1 and dev[0][b] == -1e15 and np.all(dev[1][b] == 1e15) and np.all(dev[3][b, :off[2]] == 0.0)
        for a, b in zip(dev, good):
            assert np.array_equal(bits(a[keep]), bits(b[keep]))
    engine.set_swd_search("reference")
    engine.set_swd_arith("exact")
    # bh_evaluate_batch on the same engine never reads the table
    after = engine.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True)
    for a, b in zip(after, batch0):
        assert np.array_equal(bits(a), bits(b))


def test_a_call_at_few_trials_falls_back_to_the_group_kernel_where_the_rows_do_not_fit(engine):
    """4 trials per round = 16 models per wavefront: with a row of 60 periods per model, arrays of 16 layers ask for 86 KB of LDS
    per workgroup (58 KB with one shared row), so the sites call takes the group kernel where a one-site call takes the
    trial-per-lane kernel; with arrays of 8 layers, or 8 trials, both take the trial-per-lane kernel.  Flags are the same
    either way and velocities within the default path's 2e-6."""
    rs = np.random.RandomState(9)
    descs = site_descs("nocorr_exp", rs)
    nlay, h, vp, vs, rho = synth_models(rs, B_MODELS, 16, ragged=True)
    site = (rs.permutation(B_MODELS) % NSITES).astype(np.int32)
    noise = np.tile([0.0, 0.05, 0.4, 0.05], (B_MODELS, 1))
    try:
        for trials, want in ((4, "group"), (8, "lean")):
            configure(engine, "default", trials)
            assert lean_fits(trials, 16, 60, False) and lean_fits(trials, 16, 60, True) == (want == "lean")
            engine.set_targets(descs[4])
            ref = engine.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True)
            assert engine.last_swd_kernel() == "lean"
            n, off = register(engine, descs)
            got = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
            assert engine.last_swd_kernel() == want
            m = site == 4
            assert np.array_equal(got[2][m], ref[2][m])
            a, b = got[3][m][:, :120], ref[3][m]
            assert np.array_equal(a == 0, b == 0)
            both = b != 0
            assert np.max(np.abs(a[both] - b[both]) / np.abs(b[both])) <= 2e-6
            if want == "lean":
                assert_site_bits(got, ref, m, n[4], off, "8 trials, 16 layers")
    finally:
        engine.set_swd_trials(0)


# ---- group velocities and higher modes beside per-site phase velocities ---------------------------------
def mixed_site(g, s, kind):
    """Rayleigh phase velocities at the site's own periods beside a target every site shares x on: Love group velocities
    ("group") or Rayleigh phase velocities of the first higher mode ("mode2")"""
    rs = np.random.RandomState(500 + s)
    x = PERIOD_SETS[s]
    t1 = bh.RayleighDispersionPhase(x, 3.0 + 0.3 * np.log(x) + rs.normal(0, 0.05, x.size))
    xs = np.linspace(3.0, 30.0, 12)
    if kind == "group":
        t2 = bh.LoveDispersionGroup(xs, 3.2 + 0.02 * xs + rs.normal(0, 0.05, xs.size))
    else:
        t2 = bh.RayleighDispersionPhase(xs, 4.0 + 0.02 * xs + rs.normal(0, 0.05, xs.size))
        t2.moddata.plugin.set_modelparams(mode=2)
    t1.set_noise_law("nocorr")
    t2.set_noise_law("exp")
    return bh.JointTarget([t1, t2])


@pytest.mark.parametrize("kind", ["group", "mode2"])
def test_shared_group_velocity_and_higher_mode_targets_beside_per_site_periods(engine, kind):
    """SiteTargets(per_site_x=True) with a target whose x every site shares because per-site periods are not built for it: each
    site's models equal that site's own JointTarget.evaluate_batch bit for bit, with the reference's sequence and with the
    defaults (the short refinement serves the phase-velocity target; nothing in such a call takes the fast arithmetic)."""
    nlay, h, vp, vs, rho, site = batch("synth", 21)
    S = 5
    site = (site % S).astype(np.int32)
    rs = np.random.RandomState(2)
    noise = np.column_stack([np.zeros(B_MODELS), rs.uniform(0.02, 0.1, B_MODELS), rs.uniform(0.2, 0.8, B_MODELS), rs.uniform(0.02, 0.1, B_MODELS)])
    sites = [mixed_site(None, s, kind) for s in range(S)]
    for jt in sites:
        jt._engine = engine
    st = bh.SiteTargets(sites, engine=engine, per_site_x=True)
    cap = max(x.size for x in PERIOD_SETS[:S])
    off = [0, cap, cap + 12]
    for setting in ("reference", "default"):
        configure(engine, setting, 0)
        got = st.evaluate_batch(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
        assert engine.last_swd_kernel() == "group"
        assert got[3].shape == (B_MODELS, off[-1])
        nfail = 0
        for s in range(S):
            ref = sites[s].evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True)
            m = site == s
            assert_site_bits(got, ref, m, (PERIOD_SETS[s].size, 12), off, "%s %s, site %d" % (kind, setting, s))
            nfail += int((got[2][m] != 0).sum())
        assert nfail < 0.5 * B_MODELS


# ---- chains ----------------------------------------------------------------------------------------------
PRIORS = dict(vpvs=(1.4, 2.1), layers=(1, 10), vs=(2, 5), z=(0, 60), rfnoise_corr=(0.35, 0.75),
              rfnoise_sigma=(1e-5, 0.05), swdnoise_corr=0., swdnoise_sigma=(1e-5, 0.1))
CHAIN_K = (21, 12, 30, 5)           # periods of the four sites
CHAIN_P = (5.5, 6.4, 7.5, 6.0)


def chain_site(g, s):
    rs = np.random.RandomState(300 + s)
    xs = np.asarray(g["xsw"], dtype=float)
    x = np.linspace(xs.min() + 0.3 * s, xs.max() - 1.1 * s, CHAIN_K[s])
    y = np.interp(x, xs, np.asarray(g["ysw"], dtype=float))
    t1 = bh.RayleighDispersionPhase(x, y + rs.normal(0, 0.02, x.size))
    t2 = bh.LoveDispersionPhase(x, 1.08 * y + rs.normal(0, 0.02, x.size))
    t3 = bh.PReceiverFunction(g["xrf"], g["yrf"] + rs.normal(0, 0.01, g["yrf"].size))
    t3.moddata.plugin.set_modelparams(gauss=1.0, p=CHAIN_P[s])
    return bh.JointTarget([t1, t2, t3])


class _RefUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if module.startswith("BayHunter"):
            return type(name, (object,), {})
        return super().find_class(module, name)


@pytest.mark.parametrize("depth", [None, 1])
def test_per_site_x_chains_walk_the_one_site_trajectories(depth, tmp_path):
    g = golden("chain_golden.npz")
    S, C = 4, 4
    init = dict(nchains=1, iter_burnin=150, iter_main=75, acceptance=(40, 80), thickmin=0.1, lvz=0.1, hvz=None, rcond=None,
                maxmodels=15, savepath=str(tmp_path / "multi"))
    st = bh.SiteTargets([chain_site(g, s) for s in range(S)], names=["st%d" % s for s in range(S)], per_site_x=True, per_site_rf=True)
    dc = DeviceChains(st, C, init, PRIORS, seed=77, spec_depth=depth).run()
    for s in range(S):
        one = DeviceChains(chain_site(g, s), C, init, PRIORS, seed=77, chain_offset=s * C, spec_depth=depth).run()
        for phase in ("p1", "p2"):
            a, b = dc.samples(phase, site=s), one.samples(phase)
            assert set(a) == set(b)
            for k in a:
                assert np.array_equal(a[k], b[k], equal_nan=True), "site %d %s: %s" % (s, phase, k)
    if depth is None:
        paths = dc.save()
        for s in range(S):
            with open("%s/st%d_config.pkl" % (paths[s], s), "rb") as f:
                cfg = _RefUnpickler(f).load()
            for t in range(2):      # every site's result files hold its own periods
                assert np.array_equal(cfg["targets"][t].obsdata.x, st.site(s).targets[t].obsdata.x)
                assert np.size(cfg["targets"][t].obsdata.x) == CHAIN_K[s]
            assert cfg["targets"][2].moddata.plugin.modelparams["p"] == CHAIN_P[s]
