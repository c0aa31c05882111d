"""Dispersion periods per site on EVERY dispersion target, on the MI355X (include/bh_engine_sites_x_all.h,
SiteTargets(per_site_x="all")): group velocities and higher modes at each site's own periods against each site's own
bh_evaluate_batch and against the oracle, bit for bit; the launch of second roots at each model's own periods (the site-period
build of swd_kernel) against the same call in one launch; independence of the batch's order and composition; the entry point's
refusals and lifetime; DeviceChains over sites whose phase and group curves differ in their periods against one-site runs."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import golden, REPO
import bayhunter_amd as bh
from bayhunter_amd import engine as E
from bayhunter_amd.device_chains import DeviceChains
from test_gpu_sites import eval_device
from bayhunter_amd.synth import synth_models
from test_gpu_sites_x import (batch, tables, bits, assert_site_bits, configure, PERIOD_SETS, NSITES, SITE_P, B_MODELS, FAMILIES,
                              PRIORS, X30)

pytestmark = pytest.mark.gpu

# The cases: per dispersion target (iwave, igr, mode, shift) -- site s has the periods PERIOD_SETS[(s + shift) % NSITES] x scale,
# so that two targets of a site differ in their counts where shift != 0 -- a P receiver function with its own ray parameter
# per site (rf), and the array sizes.  Higher modes: periods x 0.25 and no arrays of 8 layers -- with the periods as they are,
# or on arrays of 8 layers, most of a higher-mode row is zeros (the mode does not exist there); tests/test_sites_x_all_host.py
# asserts with the oracle that no (batch, site, target) used here is about zero rows.
CASES = {
    "group": dict(targets=[(2, 1, 1, 0), (1, 1, 1, 0)], scale=1.0, rf=False, lmax=(8, 21, 40)),
    "mixed": dict(targets=[(2, 0, 1, 0), (1, 1, 1, 2)], scale=1.0, rf=True, lmax=(8, 21, 40)),
    "mode2": dict(targets=[(2, 0, 2, 0), (1, 0, 2, 0)], scale=0.25, rf=False, lmax=(21, 40)),
    "mode2g": dict(targets=[(2, 1, 2, 0)], scale=0.25, rf=False, lmax=(21, 40)),
}
CASE_PARAMS = [(case, family, Lmax) for case, c in CASES.items() for family in FAMILIES for Lmax in c["lmax"]]
# noise laws of the dispersion targets, target after target (a case of one target takes the first)
LAW_VARIANTS = {"nocorr_exp": (E.LAW_NOCORR, E.LAW_EXP), "exp_scaled": (E.LAW_EXP, E.LAW_NOCORR_SCALED),
                "scaled": (E.LAW_NOCORR_SCALED, E.LAW_NOCORR_SCALED)}


def case_periods(case, s, t):
    iwave, igr, mode, shift = CASES[case]["targets"][t]
    return PERIOD_SETS[(s + shift) % NSITES] * CASES[case]["scale"]


def site_descs_all(case, variant, rs):
    """every site's own one-site descriptors of a case"""
    out = []
    for s in range(NSITES):
        ds = []
        for t, (iwave, igr, mode, shift) in enumerate(CASES[case]["targets"]):
            per = case_periods(case, s, t)
            n, law = per.size, LAW_VARIANTS[variant][t]
            d = dict(kind=E.TARGET_SWD, law=law, n=n, x=per, iwave=iwave, igr=igr, mode=mode,
                     yobs=3.0 + 0.3 * np.log(per / CASES[case]["scale"]) + rs.normal(0, 0.05, n))
            if law == E.LAW_NOCORR_SCALED:
                d["yerr"] = rs.uniform(0.01, 0.05, n)
            ds.append(d)
        if CASES[case]["rf"]:
            ds.append(dict(kind=E.TARGET_RF, law=E.LAW_EXP, n=150, waveno=0, nsamp=512, p=float(SITE_P[s]), gauss=2.5, fsamp=5.0,
                           tshift=5.0, nsv=0.0, yobs=rs.normal(0, 0.05, 150)))
        out.append(ds)
    return out


def register_all(eng, descs):
    """capacity descriptors (placeholders on every dispersion target), the table through bh_sites_set_x_all"""
    caps, n, x, yobs, yerr, p, nsv, off = tables(descs)
    eng.set_targets(caps)
    eng.set_sites_x_all(n, x, yobs, yerr)
    if any(d["kind"] == E.TARGET_RF for d in descs[0]):
        eng.set_sites_rf(p, nsv)
    return n, off


def noise_of(descs, rs, B=B_MODELS):
    nt = len(descs[0])
    noise = np.column_stack([rs.uniform(0.1, 0.6, B) if i % 2 == 0 else rs.uniform(0.02, 0.1, B) for i in range(2 * nt)])
    for t, d in enumerate(descs[0]):
        if d["law"] != E.LAW_EXP:
            noise[:, 2 * t] = 0.0
    return noise


def second_launches(launches):
    return [l for l in launches if l["role"] == "second"]


@pytest.mark.parametrize("case,family,Lmax", CASE_PARAMS)
def test_every_site_equals_its_own_one_site_evaluation(engine, case, family, Lmax):
    """logL, misfits, err and the whole ymod row -- zero padding and failed models included -- of evaluate_sites (host and
    device memory) equal each site's own evaluate_batch with that site's own descriptors, bit for bit."""
    nlay, h, vp, vs, rho, site = batch(family, Lmax)
    mods = (nlay, h, vp, vs, rho)
    ndisp = len(CASES[case]["targets"])
    for variant in LAW_VARIANTS:
        rs = np.random.RandomState(Lmax + 17 * len(case) + len(family) + len(variant))
        descs = site_descs_all(case, variant, rs)
        noise = noise_of(descs, rs)
        for setting in ("reference", "default"):
            what = "%s %s %s Lmax %d, %s" % (case, variant, family, Lmax, setting)
            configure(engine, setting, 0)
            refs = []
            for ds in descs:
                engine.set_targets(ds)
                refs.append(engine.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True))
            n, off = register_all(engine, descs)
            got = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
            assert engine.last_swd_kernel() == "group", what          # (no lean or one-lane-per-model main launch of such a call)
            dev = eval_device(engine, mods, noise, site, engine.ldy)
            assert engine.ldy == off[-1] and got[3].shape == (B_MODELS, off[-1])
            covered = np.zeros(B_MODELS, bool)
            for s in range(NSITES):
                m = site == s
                covered |= m
                assert_site_bits(got, refs[s], m, n[s], off, "%s, site %d host" % (what, s))
                assert_site_bits(dev, refs[s], m, n[s], off, "%s, site %d device" % (what, s))
                for t in range(ndisp):
                    assert np.all(got[3][m, off[t] + n[s, t]:off[t + 1]] == 0.0)
            assert covered.all()
            ok = got[2] == 0
            assert ok.sum() > 0.5 * B_MODELS and np.isfinite(got[0][ok]).all(), what


@pytest.mark.parametrize("case,family,Lmax", CASE_PARAMS)
def test_against_the_oracle_bit_for_bit(engine, oracle, case, family, Lmax):
    """The velocities of every site's models equal oracle.swd_batch at that site's periods, bit for bit under either setting
    (group velocities and higher modes keep the reference's sequence and arithmetic; the phase-velocity target of "mixed"
    does so with search = "reference"), failure flags and zero rows included."""
    rs = np.random.RandomState(60 + Lmax)
    descs = site_descs_all(case, "nocorr_exp", rs)
    nlay, h, vp, vs, rho, site = batch(family, Lmax)
    noise = noise_of(descs, rs)
    want = {}
    for s in range(NSITES):
        m = site == s
        for t, (iwave, igr, mode, shift) in enumerate(CASES[case]["targets"]):
            want[s, t] = oracle.swd_batch(nlay[m], h.T[m], vp.T[m], vs.T[m], rho.T[m], case_periods(case, s, t), iwave, igr, mode=mode)[:2]
    for setting in ("reference", "default"):
        configure(engine, setting, 0)
        n, off = register_all(engine, descs)
        logL, misf, err, ymod = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
        for s in range(NSITES):
            m = site == s
            bad = np.zeros(m.sum(), bool)
            for t, (iwave, igr, mode, shift) in enumerate(CASES[case]["targets"]):
                v, e = want[s, t]
                bad |= e != 0
                if igr == 0 and mode == 1 and setting != "reference":
                    continue          # (the short refinement: within 2.5e-6, tests/test_gpu_sites_x.py)
                assert np.array_equal(bits(ymod[m, off[t]:off[t] + n[s, t]]), bits(v)), (case, family, Lmax, setting, s, t)
            assert np.array_equal(err[m] != 0, bad), (case, family, Lmax, setting, s)
            assert np.all(logL[m][bad] == -1e15)


def _split_off_rows(case, family, Lmax):
    """(run in a child process started with BH_SWD_GSPLIT=0) the rows of the call of test_the_second_roots_... in one launch"""
    eng = E.default_engine(0)
    eng.set_swd_search("reference")
    eng.set_swd_arith("exact")
    assert eng.tuning("swd_gsplit") == 0
    rs = np.random.RandomState(23)
    descs = site_descs_all(case, "nocorr_exp", rs)
    nlay, h, vp, vs, rho, site = batch(family, Lmax)
    noise = noise_of(descs, rs)
    register_all(eng, descs)
    got = eng.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
    assert not second_launches(eng.last_swd_launches())
    return got


@pytest.mark.parametrize("case,family,Lmax", [("group", "prior", 21), ("mixed", "synth", 8)])
def test_the_second_roots_run_in_their_own_launch_and_equal_the_unsplit_call(engine, tmp_path, case, family, Lmax):
    """A split call lists one "second" launch of family "lane" per group-velocity target -- the site-period build of swd_kernel --
    and its rows equal those of the same call with the split off (BH_SWD_GSPLIT=0, read when a process first uses the
    library: a fresh child process)."""
    assert engine.tuning("swd_gsplit") == 1 << 24
    rs = np.random.RandomState(23)
    descs = site_descs_all(case, "nocorr_exp", rs)
    nlay, h, vp, vs, rho, site = batch(family, Lmax)
    noise = noise_of(descs, rs)
    configure(engine, "reference", 0)
    register_all(engine, descs)
    got = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
    launches = engine.last_swd_launches()
    ngroup = sum(1 for tg in CASES[case]["targets"] if tg[1] == 1)
    sec = second_launches(launches)
    assert len(sec) == ngroup and all(l["family"] == "lane" for l in sec), launches
    # (the instantiation: reference sequence, not SIMPLE, no fast arithmetic)
    assert all(tuple(l["key"][3:]) == (0, 0, 0) for l in sec), sec
    assert sorted(l["key"][0] for l in sec) == sorted(tg[0] for tg in CASES[case]["targets"] if tg[1] == 1)
    out = str(tmp_path / "unsplit.npz")
    code = ("import sys; sys.path[:0] = [%r, %r]; import numpy as np; import test_gpu_sites_x_all as T; "
            "g = T._split_off_rows(%r, %r, %d); np.savez(%r, logL=g[0], misf=g[1], err=g[2], ymod=g[3])"
            % (REPO, os.path.join(REPO, "tests"), case, family, Lmax, out))
    env = dict(os.environ, BH_SWD_GSPLIT="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    one = np.load(out)
    for a, k in zip(got, ("logL", "misf", "err", "ymod")):
        assert np.array_equal(bits(a), bits(one[k])), k
    assert (got[2] == 0).sum() > 0.5 * B_MODELS


# One lane per search (more than 2048 x 64 / 16 searches in the call), in both time-slice classes: 2200 models x 60 periods are
# 2063 wavefronts (two per workgroup), 1500 x 60 are 1407 (one per workgroup) -- the builds the batches above, whose searches
# get trial lanes, do not reach.  (Trial lanes with two wavefronts per workgroup are compiled but never chosen: the trial lanes
# are sized so that the call's searches fit 2048 wavefronts.)
BIG_SHAPES = [(2200, 2), (1500, 1)]


def big_batch(B):
    rs = np.random.RandomState(900 + B)
    mods = synth_models(rs, B, 12, ragged=True)
    return mods + ((rs.permutation(B) % NSITES).astype(np.int32),)


@pytest.mark.parametrize("iwave", [2, 1])
@pytest.mark.parametrize("B,wpb", BIG_SHAPES)
def test_one_lane_per_second_root_in_both_workgroup_sizes(engine, oracle, B, wpb, iwave):
    nlay, h, vp, vs, rho, site = big_batch(B)
    rs = np.random.RandomState(B + iwave)
    descs = [[dict(kind=E.TARGET_SWD, law=E.LAW_EXP, n=per.size, x=per, iwave=iwave, igr=1, yobs=3.0 + 0.3 * np.log(per) + rs.normal(0, 0.05, per.size))]
             for per in PERIOD_SETS]
    noise = noise_of(descs, rs, B)
    configure(engine, "reference", 0)
    n, off = register_all(engine, descs)
    logL, misf, err, ymod = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
    sec = second_launches(engine.last_swd_launches())
    assert len(sec) == 1 and sec[0]["family"] == "lane" and tuple(sec[0]["key"]) == (iwave, 0, wpb, 0, 0, 0), sec
    for s, per in enumerate(PERIOD_SETS):
        m = site == s
        v, e, _ = oracle.swd_batch(nlay[m], h.T[m], vp.T[m], vs.T[m], rho.T[m], per, iwave, 1)
        assert np.array_equal(bits(ymod[m, :per.size]), bits(v)) and np.all(ymod[m, per.size:] == 0.0), (B, iwave, s)
        assert np.array_equal(err[m] != 0, e != 0)
    assert (err == 0).sum() > 0.5 * B


@pytest.mark.parametrize("case,setting,Lmax", [("group", "reference", 21), ("mixed", "default", 8), ("mode2g", "default", 40)])
def test_results_do_not_depend_on_order_numbering_or_company(engine, case, setting, Lmax):
    rs = np.random.RandomState(31 + Lmax)
    descs = site_descs_all(case, "exp_scaled", rs)
    nlay, h, vp, vs, rho, site = batch("prior", Lmax)
    noise = noise_of(descs, rs)
    configure(engine, setting, 0)
    register_all(engine, descs)
    base = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
    q = rs.permutation(B_MODELS)                         # the batch permuted
    got = engine.evaluate_sites(nlay[q], h[:, q], vp[:, q], vs[:, q], noise[q], site[q], rho=rho[:, q], want_ymod=True)
    for a, b in zip(got, base):
        assert np.array_equal(bits(a), bits(b[q])), "permuted"
    r = rs.permutation(NSITES)                           # the sites renumbered: new number of site s = r[s]
    inv = np.argsort(r)
    register_all(engine, [descs[inv[k]] for k in range(NSITES)])
    got = engine.evaluate_sites(nlay, h, vp, vs, noise, r[site].astype(np.int32), rho=rho, want_ymod=True)
    for a, b in zip(got, base):
        assert np.array_equal(bits(a), bits(b)), "renumbered"
    if not (setting == "default" and case == "mixed"):   # (the short refinement's bits follow the plan of the call's shape)
        register_all(engine, descs)
        for s in (1, 3, 4):                              # one site's models alone in the call
            m = site == s
            got = engine.evaluate_sites(nlay[m], h[:, m], vp[:, m], vs[:, m], noise[m], site[m], rho=rho[:, m], want_ymod=True)
            for a, b in zip(got, base):
                assert np.array_equal(bits(a), bits(b[m])), "site %d alone" % s


def test_shared_periods_through_the_table_equal_the_shared_x_path(engine):
    """Sites that share their group-velocity periods: the table of bh_sites_set_x_all, the table of bh_sites_set_x (which
    searches the second roots at the descriptor's periods) and the plain site table return the same bits."""
    rs = np.random.RandomState(8)
    same = [[dict(kind=E.TARGET_SWD, law=law, n=30, x=X30, iwave=iw, igr=1, yobs=3.0 + 0.3 * np.log(X30) + rs.normal(0, 0.05, 30))
             for iw, law in ((2, E.LAW_NOCORR), (1, E.LAW_EXP))] for s in range(NSITES)]
    nlay, h, vp, vs, rho, site = batch("synth", 21)
    noise = noise_of(same, rs)
    caps, n, x, yobs, yerr, p, nsv, off = tables(same)
    engine.set_targets(same[0])
    engine.set_sites(yobs, yerr)
    plain = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
    engine.set_sites_x(n, x, yobs, yerr)
    old = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
    register_all(engine, same)
    new = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
    assert len(second_launches(engine.last_swd_launches())) == 2
    for a, b, c in zip(plain, old, new):
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))


def test_api_refusals_lifetime_and_in_band_failure(engine):
    rs = np.random.RandomState(4)
    descs = site_descs_all("mixed", "exp_scaled", rs)
    nlay, h, vp, vs, rho, site = batch("synth", 21)
    B = 120
    nlay, h, vp, vs, rho, site = nlay[:B], h[:, :B], vp[:, :B], vs[:, :B], rho[:, :B], site[:B]
    noise = noise_of(descs, rs, B)
    caps, n, x, yobs, yerr, p, nsv, off = tables(descs)
    L, hd = engine._L, engine._h
    P = lambda a: a.ctypes.data
    S = NSITES

    def rc(n_=n, x_=x, yobs_=yobs, yerr_=yerr, S_=S, entry=L.bh_sites_set_x_all):
        return entry(hd, S_, P(n_) if n_ is not None else None, P(x_) if x_ is not None else None,
                     P(yobs_) if yobs_ is not None else None, P(yerr_) if yerr_ is not None else None)

    engine.set_targets(caps)
    batch0 = engine.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True)
    assert rc() == E.BH_OK
    # the same tables through bh_sites_set_x: per-site periods on a group-velocity target are not built there
    engine.set_targets(caps)
    assert rc(entry=L.bh_sites_set_x) == E.BH_EUNSUPPORTED
    assert b"bh_sites_set_x:" in L.bh_engine_last_error(hd)
    with pytest.raises(E.EngineError, match="site table"):      # nothing is registered by a refused call
        engine.set_sites_rf(p, nsv)
    # null arguments, a count below 1 or above the capacity, periods that are not finite and positive, an RF count
    assert rc(n_=None) == E.BH_EINVAL and rc(x_=None) == E.BH_EINVAL and rc(yobs_=None) == E.BH_EINVAL
    assert b"bh_sites_set_x_all" in L.bh_engine_last_error(hd)
    assert rc(yerr_=None) == E.BH_EINVAL            # a scaled-error target needs yerr
    assert rc(S_=0) == E.BH_EINVAL
    for bad in (0, -3, 61):
        b = n.copy()
        b[2, 1] = bad                               # (the group-velocity target)
        assert rc(n_=b) == E.BH_EINVAL, bad
    b = n.copy()
    b[1, 2] -= 1                                    # a receiver function's count is its descriptor's
    assert rc(n_=b) == E.BH_EINVAL
    for bad in (0.0, -2.0, np.nan, np.inf):
        b = x.copy()
        b[1, off[1] + n[1, 1] - 1] = bad            # (the last period site 1 has on the group-velocity target)
        assert rc(x_=b) == E.BH_EINVAL, bad
    b = x.copy()
    b[1, off[1] + n[1, 1]] = np.nan                 # beyond a site's own count nothing is read
    assert rc(x_=b) == E.BH_OK
    # the Gauss law on a dispersion target; more than 60 periods
    g = [dict(d) for d in caps]
    g[1].update(law=E.LAW_GAUSS, rinv=np.eye(g[1]["n"]), logdet_r=0.0)
    engine.set_targets(g)
    assert rc() == E.BH_EINVAL
    big = [dict(kind=E.TARGET_SWD, law=E.LAW_NOCORR, n=61, x=np.linspace(2, 60, 61), iwave=2, igr=1, yobs=np.zeros(61))]
    engine.set_targets(big)
    assert L.bh_sites_set_x_all(hd, 1, P(np.array([[61]], np.int32)), P(np.linspace(2, 60, 61)[None].copy()), P(np.zeros((1, 61))), None) == E.BH_EUNSUPPORTED
    # every dispersion target the engine serves is accepted: modes 1 to 3, flattened, either velocity and wave type
    for change in (dict(mode=2), dict(mode=3, igr=1), dict(flsph=1), dict(iwave=1, igr=0, mode=2, flsph=1)):
        g = [dict(d) for d in caps]
        g[1].update(change)
        engine.set_targets(g)
        assert rc() == E.BH_OK, change
    # lifetime: bh_sites_set, bh_sites_set_x and bh_targets_set drop the table, bh_sites_set_rf may follow it
    engine.set_targets(caps)
    engine.set_sites_x_all(n, x, yobs, yerr)
    engine.set_sites_rf(p, nsv)
    own = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
    assert len(second_launches(engine.last_swd_launches())) == 1
    engine.set_sites(yobs, yerr)                    # the plain table: the descriptors' placeholder periods (1 s) at every site
    plain = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
    assert not np.array_equal(plain[3][:, :off[2]], own[3][:, :off[2]])
    engine.set_sites_x_all(n, x, yobs, yerr)
    engine.set_sites_rf(p, nsv)
    again = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
    for a, b in zip(again, own):
        assert np.array_equal(bits(a), bits(b))
    engine.set_targets(caps)
    with pytest.raises(E.EngineError, match="site table"):
        engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho)
    # a device-side site out of range fails in band and reads nothing; the others are untouched -- with the second roots in
    # their own launch and, many more (model, period) pairs than the split's limit, in the chain's
    engine.set_sites_x_all(n, x, yobs, yerr)
    engine.set_sites_rf(p, nsv)
    wild = site.copy()
    wild[5], wild[17] = NSITES, -1
    keep = np.ones(B, bool)
    keep[[5, 17]] = False
    try:
        for gsplit in (1 << 24, 0):
            engine.set_tuning("swd_gsplit", gsplit)
            dev = eval_device(engine, (nlay, h, vp, vs, rho), noise, wild, engine.ldy)
            assert len(second_launches(engine.last_swd_launches())) == (1 if gsplit else 0)
            for b in (5, 17):
                assert dev[2][b] == 1 and dev[0][b] == -1e15 and np.all(dev[1][b] == 1e15) and np.all(dev[3][b, :off[2]] == 0.0)
            for a, b in zip(dev, own):
                assert np.array_equal(bits(a[keep]), bits(b[keep]))
    finally:
        engine.set_tuning("swd_gsplit", 1 << 24)
    with pytest.raises(E.EngineError, match="out of range"):    # host memspace: checked before anything is launched
        engine.evaluate_sites(nlay, h, vp, vs, noise, wild, rho=rho)
    # bh_evaluate_batch on the same engine never reads the table
    engine.set_targets(caps)
    engine.set_sites_x_all(n, x, yobs, yerr)
    after = engine.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True)
    for a, b in zip(after, batch0):
        assert np.array_equal(bits(a), bits(b))


# ---- chains ----------------------------------------------------------------------------------------------
CHAIN_KP = (21, 12, 30, 5)          # periods of the four sites' phase-velocity curves
CHAIN_KG = (9, 26, 14, 30)          # ... and of their group-velocity curves
CHAIN_P = (5.5, 6.4, 7.5, 6.0)


def chain_site_all(g, s):
    """Rayleigh phase + Rayleigh group velocities + a P receiver function; period counts differ per target and per site"""
    rs = np.random.RandomState(400 + s)
    xs = np.asarray(g["xsw"], dtype=float)
    ys = np.asarray(g["ysw"], dtype=float)
    x1 = np.linspace(xs.min() + 0.3 * s, xs.max() - 1.1 * s, CHAIN_KP[s])
    x2 = np.linspace(xs.min() + 0.7 * s, xs.max() - 0.4 * s, CHAIN_KG[s])
    t1 = bh.RayleighDispersionPhase(x1, np.interp(x1, xs, ys) + rs.normal(0, 0.02, x1.size))
    t2 = bh.RayleighDispersionGroup(x2, 0.9 * np.interp(x2, xs, ys) + rs.normal(0, 0.02, x2.size))
    t3 = bh.PReceiverFunction(g["xrf"], g["yrf"] + rs.normal(0, 0.01, g["yrf"].size))
    t3.moddata.plugin.set_modelparams(gauss=1.0, p=CHAIN_P[s])
    return bh.JointTarget([t1, t2, t3])


@pytest.mark.parametrize("depth", [None, 1])
def test_per_site_x_all_chains_walk_the_one_site_trajectories(depth, tmp_path):
    g = golden("chain_golden.npz")
    S, C = 4, 4
    init = dict(nchains=1, iter_burnin=150, iter_main=75, acceptance=(40, 80), thickmin=0.1, lvz=0.1, hvz=None, rcond=None,
                maxmodels=15, savepath=str(tmp_path / "multi"))
    st = bh.SiteTargets([chain_site_all(g, s) for s in range(S)], names=["st%d" % s for s in range(S)], per_site_x="all", per_site_rf=True)
    dc = DeviceChains(st, C, init, PRIORS, seed=77, spec_depth=depth).run()
    for s in range(S):
        one = DeviceChains(chain_site_all(g, s), C, init, PRIORS, seed=77, chain_offset=s * C, spec_depth=depth).run()
        for phase in ("p1", "p2"):
            a, b = dc.samples(phase, site=s), one.samples(phase)
            assert set(a) == set(b)
            for k in a:
                assert np.array_equal(a[k], b[k], equal_nan=True), "site %d %s: %s" % (s, phase, k)
