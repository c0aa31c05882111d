"""Many stations at once on the MI355X (include/bh_engine_sites.h, bayhunter_amd/sites.py): bh_evaluate_sites against each
site's own bh_evaluate_batch, bit for bit, and DeviceChains over SiteTargets against one-site runs."""
import os

import numpy as np
import pytest

from conftest import golden
import bayhunter_amd as bh
import like_ref as LR
from bayhunter_amd import engine as E
from bayhunter_amd.device_chains import DeviceChains
from bayhunter_amd.synth import synth_models
from bayhunter_amd.Targets import Valuation

pytestmark = pytest.mark.gpu

PER = np.linspace(2.0, 60.0, 30)
PER75 = np.linspace(3.0, 80.0, 75)


def rinv_of(n, corr=0.9):
    return np.ascontiguousarray(Valuation.get_corr_inv(corr, n) / (1.0 - corr * corr)), float((n - 1) * np.log(1.0 - corr * corr))


def structure(case):
    """target descriptors without observed data: (kind, law, n, extra)"""
    rf = dict(kind=E.TARGET_RF, nsamp=512, p=6.4, gauss=2.5, fsamp=5.0, tshift=5.0)
    if case == "laws":      # all four laws, dispersion (phase, group) beside a P receiver function
        return [dict(kind=E.TARGET_SWD, law=E.LAW_NOCORR, n=30, x=PER, iwave=2, igr=0),
                dict(kind=E.TARGET_SWD, law=E.LAW_NOCORR_SCALED, n=30, x=PER, iwave=1, igr=0),
                dict(kind=E.TARGET_SWD, law=E.LAW_EXP, n=30, x=PER, iwave=2, igr=1),
                dict(rf, law=E.LAW_GAUSS, n=30, waveno=0)]
    if case == "rf":        # P and SV receiver functions (exponential: fused on the one-site path), Love group velocities
        return [dict(rf, law=E.LAW_EXP, n=201, waveno=0), dict(rf, law=E.LAW_NOCORR, n=201, waveno=1, p=7.0),
                dict(kind=E.TARGET_SWD, law=E.LAW_EXP, n=30, x=PER, iwave=1, igr=1)]
    if case == "long":      # > 60 periods (interpolated), scaled errors
        return [dict(kind=E.TARGET_SWD, law=E.LAW_NOCORR_SCALED, n=75, x=PER75, iwave=2, igr=0),
                dict(kind=E.TARGET_SWD, law=E.LAW_EXP, n=75, x=PER75, iwave=1, igr=0)]
    if case == "gauss1024":  # a long Gauss-law receiver function: the contraction form follows from B (see the parametrisation)
        return [dict(rf, law=E.LAW_GAUSS, n=1024, nsamp=2048, fsamp=20.0, waveno=0)]
    raise KeyError(case)


def site_descs(case, S, rs):
    """S sites of one structure: observed data (and yerr) per site"""
    base = structure(case)
    out = []
    for s in range(S):
        ds = []
        for d in base:
            d = dict(d)
            n = d["n"]
            if d["kind"] == E.TARGET_SWD:
                d["yobs"] = 3.0 + 0.02 * np.arange(n) / n * 30 + rs.normal(0, 0.05, n)
            else:
                d["yobs"] = rs.normal(0, 0.05, n)
            if d["law"] == E.LAW_NOCORR_SCALED:
                d["yerr"] = rs.uniform(0.01, 0.2, n)
            if d["law"] == E.LAW_GAUSS:
                d["rinv"], d["logdet_r"] = rinv_of(n)
            ds.append(d)
        out.append(ds)
    return out


def table(descs):
    yobs = np.vstack([np.concatenate([d["yobs"] for d in ds]) for ds in descs])
    yerr = np.vstack([np.concatenate([d.get("yerr", np.ones(d["n"])) for d in ds]) for ds in descs])
    return yobs, yerr


def batch(rs, B, nt):
    nlay, h, vp, vs, rho = synth_models(rs, B, 10, ragged=True)
    vs[0, ::7] = 9.0        # a few failing models (no root: the top layer faster than the half-space...)
    noise = np.column_stack([rs.uniform(0.1, 0.6, B) if i % 2 == 0 else rs.uniform(0.02, 0.1, B) for i in range(2 * nt)])
    return nlay, h, vp, vs, rho, noise


def per_site(eng, descs, models, noise):
    """every model evaluated with each site's own targets (the whole batch: the same launch shapes)"""
    out = []
    for ds in descs:
        eng.set_targets(ds)
        out.append(eng.evaluate_batch(*models[:4], noise, rho=models[4], want_ymod=True))
    return out


def assert_sites_equal(got, refs, site, what):
    logL, misf, err, ymod = got
    for s, (rl, rm, re_, ry) in enumerate(refs):
        m = site == s
        assert np.array_equal(logL[m], rl[m]), "%s: logL of site %d" % (what, s)
        assert np.array_equal(misf[m], rm[m]), "%s: misfits of site %d" % (what, s)
        assert np.array_equal(err[m], re_[m]), "%s: err of site %d" % (what, s)
        ok = m & (err == 0)
        assert np.array_equal(ymod[ok], ry[ok]), "%s: ymod of site %d" % (what, s)


def eval_device(eng, models, noise, site, ldy):
    import torch
    nlay, h, vp, vs, rho = models
    L, B = h.shape
    dev = torch.device("cuda", 0)
    T = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)
    tn, th, tvp, tvs, trho = T(nlay, torch.int32), T(h), T(vp), T(vs), T(rho)
    tsite, tnoise = T(site, torch.int32), T(noise)
    logL, misf = torch.zeros(B, dtype=torch.float64, device=dev), torch.zeros((B, len(noise[0]) // 2 + 1), dtype=torch.float64, device=dev)
    err, ymod = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros((B, ldy), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    eng.evaluate_sites_dev(B, L, tn.data_ptr(), th.data_ptr(), tvp.data_ptr(), tvs.data_ptr(), trho.data_ptr(), B, 1,
                           tsite.data_ptr(), tnoise.data_ptr(), logL.data_ptr(), misf.data_ptr(), err.data_ptr(), ymod.data_ptr())
    eng.synchronize()
    return logL.cpu().numpy(), misf.cpu().numpy(), err.cpu().numpy(), ymod.cpu().numpy()


def test_fused_receiver_function_sums_equal_the_unfused_ones(engine):
    """The sites path writes receiver functions to the ymod workspace and the likelihood kernel forms the sums; the one-site
    path fuses them into the synthesis kernel.  rf_kernel.hip says both are formed in the same order: checked bit for bit."""
    rs = np.random.RandomState(3)
    ds = site_descs("rf", 1, rs)[0]
    engine.set_targets(ds)
    nlay, h, vp, vs, rho, noise = batch(rs, 300, len(ds))
    a = engine.evaluate_batch(nlay, h, vp, vs, noise, rho=rho)
    b = engine.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True)
    for x, y in zip(a, b[:3]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("search", ["reference", "fast32"])
# The Gauss contraction (gauss_kernel.hip: use_big_tiles, big_ksplit): "laws" (n = 30) and "gauss1024" at B = 300 take the 64 x 64
# form (ceil(B/128) * ceil(n/128) < 128); "gauss1024" at B = 2048 and 4096 the 128 x 128 form, with K split over 4 and 2 workgroups.
@pytest.mark.parametrize("case,B", [("laws", 1), ("laws", 5), ("laws", 300), ("rf", 129), ("long", 65), ("gauss1024", 300),
                                    ("gauss1024", 2048), ("gauss1024", 4096), ("laws", 4097)])
def test_evaluate_sites_equals_each_sites_own_evaluation(engine, case, B, search):
    rs = np.random.RandomState(B + len(case))
    S = 5
    descs = site_descs(case, S, rs)
    nt = len(descs[0])
    nlay, h, vp, vs, rho, noise = batch(rs, B, nt)
    site = rs.choice([0, 2, 3, 4], B).astype(np.int32)      # site 1 receives no model
    models = (nlay, h, vp, vs, rho)
    ctx = engine.searching("fast") if search == "fast32" else engine.searching("reference")
    with ctx, engine.trying(32 if search == "fast32" else None):
        refs = per_site(engine, descs, models, noise)
        engine.set_targets(descs[0])
        engine.set_sites(*table(descs))
        got = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
        assert_sites_equal(got, refs, site, "%s B=%d host" % (case, B))
        dgot = eval_device(engine, models, noise, site, engine.ldy)
        assert_sites_equal(dgot, refs, site, "%s B=%d device" % (case, B))
    if any(d["kind"] == E.TARGET_SWD for d in descs[0]) and B >= 7:
        assert (got[2] != 0).any()          # (the failing models of batch(): every 7th)
    # each logL against the extended-precision reference with its own site's data; another site's data lies far outside
    logL, _, err, ymod = got
    for s in (0, 2):
        m = (site == s) & (err == 0)
        if not m.any():
            continue
        ref, _, bound, _ = LR.joint_ref(descs[s], ymod[m], noise[m])
        LR.assert_within(logL[m], ref, bound, "%s site %d" % (case, s))
        other, _, _, _ = LR.joint_ref(descs[(s + 2) % 5], ymod[m], noise[m])
        assert np.all(np.abs(logL[m] - other.astype(float)) > 1e3 * bound)


def test_gauss_in_kernel_matvec_with_sites(engine):
    """no_mfma: the likelihood kernel's own mat-vec reads each model's site row"""
    before = engine.tuning("no_mfma")
    engine.set_tuning("no_mfma", 1)
    eng = None
    try:
        eng = E.Engine(0)
        eng.set_swd_search("reference")
        rs = np.random.RandomState(5)
        descs = site_descs("laws", 3, rs)
        nlay, h, vp, vs, rho, noise = batch(rs, 129, 4)
        site = rs.randint(0, 3, 129).astype(np.int32)
        refs = per_site(eng, descs, (nlay, h, vp, vs, rho), noise)
        eng.set_targets(descs[0])
        eng.set_sites(*table(descs))
        assert_sites_equal(eng.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True), refs, site, "no_mfma")
    finally:
        if eng is not None:
            eng.close()
        engine.set_tuning("no_mfma", before)


def test_one_site_and_bad_indices(engine):
    rs = np.random.RandomState(9)
    descs = site_descs("laws", 1, rs)
    nlay, h, vp, vs, rho, noise = batch(rs, 200, 4)
    engine.set_targets(descs[0])
    ref = engine.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True)
    with pytest.raises(E.EngineError, match="site table"):
        engine.evaluate_sites(nlay, h, vp, vs, noise, np.zeros(200, np.int32), rho=rho)
    engine.set_sites(*table(descs))
    got = engine.evaluate_sites(nlay, h, vp, vs, noise, np.zeros(200, np.int32), rho=rho, want_ymod=True)
    for x, y in zip(got, ref):
        assert np.array_equal(x, y)
    bad = np.zeros(200, np.int32)
    bad[[3, 77]] = [1, -1]
    with pytest.raises(E.EngineError, match="out of range"):
        engine.evaluate_sites(nlay, h, vp, vs, noise, bad, rho=rho)
    logL, misf, err, _ = eval_device(engine, (nlay, h, vp, vs, rho), noise, bad, engine.ldy)
    assert err[3] == 1 and err[77] == 1 and logL[3] == -1e15 and np.all(misf[[3, 77]] == 1e15)
    ok = np.ones(200, bool)
    ok[[3, 77]] = False
    assert np.array_equal(logL[ok], ref[0][ok]) and np.array_equal(err[ok], ref[2][ok])
    engine.set_targets(descs[0])            # set_targets drops the site table
    with pytest.raises(E.EngineError, match="site table"):
        engine.evaluate_sites(nlay, h, vp, vs, noise, np.zeros(200, np.int32), rho=rho)


# ---- chains ----------------------------------------------------------------------------------------------
PRIORS = dict(vpvs=(1.4, 2.1), layers=(1, 10), vs=(2, 5), z=(0, 60), rfnoise_corr=(0.35, 0.75),
              rfnoise_sigma=(1e-5, 0.05), swdnoise_corr=0., swdnoise_sigma=(1e-5, 0.1))


def chain_site(g, s):
    """site s: the golden observed data with a noise draw of its own"""
    rs = np.random.RandomState(100 + s)
    t1 = bh.RayleighDispersionPhase(g["xsw"], g["ysw"] + rs.normal(0, 0.02, g["ysw"].size))
    t2 = bh.LoveDispersionPhase(g["xsw"], 1.05 * g["ysw"] + rs.normal(0, 0.02, g["ysw"].size))
    t3 = bh.PReceiverFunction(g["xrf"], g["yrf"] + rs.normal(0, 0.01, g["yrf"].size))
    t3.moddata.plugin.set_modelparams(gauss=1.0, p=6.4)
    return bh.JointTarget([t1, t2, t3])


def same_samples(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), "%s: %s" % (what, k)


@pytest.mark.parametrize("depth", [None, 1])
def test_site_chains_walk_the_one_site_trajectories(depth, tmp_path):
    g = golden("chain_golden.npz")
    S, C = 3, 4
    init = dict(nchains=1, iter_burnin=180, iter_main=90, acceptance=(40, 80), thickmin=0.1, lvz=0.1, hvz=None, rcond=None,
                maxmodels=15, savepath=str(tmp_path / "multi"))
    st = bh.SiteTargets([chain_site(g, s) for s in range(S)], names=["st%d" % s for s in range(S)])
    dc = DeviceChains(st, C, init, PRIORS, seed=123, spec_depth=depth).run()
    paths = dc.save()
    for s in range(S):
        ip = dict(init, savepath=str(tmp_path / "one" / ("st%d" % s)), station="st%d" % s)
        one = DeviceChains(chain_site(g, s), C, ip, PRIORS, seed=123, chain_offset=s * C, spec_depth=depth).run()
        for phase in ("p1", "p2"):
            same_samples(dc.samples(phase, site=s), one.samples(phase), "site %d %s" % (s, phase))
        if depth is None:
            dpath = one.save()
            files = sorted(f for f in os.listdir(dpath) if f.endswith(".npy"))
            assert files and files == sorted(f for f in os.listdir(paths[s]) if f.endswith(".npy"))
            for f in files:
                assert np.array_equal(np.load(os.path.join(dpath, f)), np.load(os.path.join(paths[s], f)), equal_nan=True), f
            assert os.path.exists(os.path.join(paths[s], "st%d_config.pkl" % s))
            bh.save_final_distribution(paths[s], maxmodels=1000)


def test_tempered_site_chains_and_ladders_across_sites():
    g = golden("chain_golden.npz")
    S, C = 2, 4
    init = dict(nchains=1, iter_burnin=120, iter_main=60, acceptance=(40, 80), thickmin=0.1, lvz=0.1, hvz=None, rcond=None,
                maxmodels=10)
    betas = np.tile([1.0, 0.8, 1.0, 0.8], S)
    ladder = np.repeat(np.arange(2 * S), 2)                 # two ladders of two rungs per site
    st = bh.SiteTargets([chain_site(g, s) for s in range(S)])
    dc = DeviceChains(st, C, init, PRIORS, seed=9, betas=betas, ladder=ladder, swap_every=5).run()
    for s in range(S):
        blk = slice(s * C, (s + 1) * C)
        one = DeviceChains(chain_site(g, s), C, init, PRIORS, seed=9, chain_offset=s * C, betas=betas[blk], ladder=ladder[blk],
                           swap_every=5).run()
        same_samples(dc.samples("p2", site=s), one.samples("p2"), "tempered site %d" % s)
        same_samples(dc.samples("p2", site=s, cold_only=True), one.samples("p2", cold_only=True), "cold site %d" % s)
    with pytest.raises(E.EngineError, match="spans sites"):
        DeviceChains(bh.SiteTargets([chain_site(g, s) for s in range(S)]), C, init, PRIORS, seed=9, betas=betas,
                     ladder=np.array([0, 0, 0, 1, 1, 1, 1, 0]), swap_every=5)
