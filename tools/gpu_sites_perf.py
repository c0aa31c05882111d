"""Chain-iterations/s of many stations at once: S sites x 8 chains in ONE DeviceChains (SiteTargets) against S one-site
DeviceChains runs made one after another, on joint Rayleigh + Love phase dispersion + P receiver function (exponential law),
prior-like transdimensional models (1..20 layers).  Only the iterations are timed (the host-built initial states are not).

    python tools/gpu_sites_perf.py [--sites 1,8,64] [--iters 300] [--out profiles/sites_perf.json]

The like / Gauss kernel times with and without sites come from a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/gpu_sites_perf.py --like-only`: 4096 models per call, each path five times, with
the exponential and the Gauss law on a 201-sample receiver function (64 x 64 contraction) and the Gauss law on a 1024-sample one
(128 x 128 contraction).

Receiver-function parameters per site (SiteTargets(per_site_rf=True), include/bh_engine_sites_rf.h):

    python tools/gpu_sites_perf.py --per-site-rf [--sites 8,64] [--out profiles/sites_rf_perf.json]

runs S sites x 8 chains three ways: every site at p = 6.4 s/deg (shared p), p spread evenly over 5..8 s/deg (per-site p), and
the S one-site runs with those p made one after another; the two site runs alternate `--repeat` times (median reported).
`rocprofv3 --kernel-trace --stats -- python tools/gpu_sites_perf.py --rf-coef-only` gives the coefficient kernels at B = 4096
with and without a table of p (Lmax 10: the 16-lane build, alone and -- beside the dispersion targets -- its _small build;
Lmax 40: the one-lane build).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bayhunter_amd as bh  # noqa: E402
from bayhunter_amd.device_chains import DeviceChains  # noqa: E402

PRIORS = dict(vpvs=(1.4, 2.1), layers=(1, 20), vs=(2, 5), z=(0, 60), rfnoise_corr=(0.35, 0.75),
              rfnoise_sigma=(1e-5, 0.05), swdnoise_corr=0., swdnoise_sigma=(1e-5, 0.1))
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "chain_golden.npz")


def site(g, s, p=6.4):
    rs = np.random.RandomState(1000 + s)
    t1 = bh.RayleighDispersionPhase(g["xsw"], g["ysw"] + rs.normal(0, 0.02, g["ysw"].size))
    t2 = bh.LoveDispersionPhase(g["xsw"], 1.05 * g["ysw"] + rs.normal(0, 0.02, g["ysw"].size))
    t3 = bh.PReceiverFunction(g["xrf"], g["yrf"] + rs.normal(0, 0.01, g["yrf"].size))
    t3.moddata.plugin.set_modelparams(gauss=1.0, p=p)
    return bh.JointTarget([t1, t2, t3])


def spread_p(S):
    """S ray parameters spread evenly over 5..8 s/deg"""
    return [5.0 + 3.0 * s / max(S - 1, 1) for s in range(S)]


def per_site_rf(a, g, init):
    res = {"chains_per_site": a.chains, "iters": a.iters, "repeat": a.repeat,
           "workload": "R+L phase dispersion (21 periods) + P-RF exp law, 1..20 layers", "runs": []}
    for S in [int(x) for x in a.sites.split(",")]:
        ps = spread_p(S)
        shared = DeviceChains(bh.SiteTargets([site(g, s) for s in range(S)]), a.chains, init, PRIORS, seed=5)
        own = DeviceChains(bh.SiteTargets([site(g, s, ps[s]) for s in range(S)], per_site_rf=True), a.chains, init, PRIORS, seed=5)
        timed(shared, a.warm)
        timed(own, a.warm)
        rs, ro = [], []
        for _ in range(a.repeat):       # alternating: drifts of the clock or the host hit both alike
            n, dt = timed(shared, a.iters)
            rs.append(n / dt)
            n, dt = timed(own, a.iters)
            ro.append(n / dt)
        seq_n, seq_dt = 0, 0.0
        for s in range(S):
            one = DeviceChains(site(g, s, ps[s]), a.chains, init, PRIORS, seed=5, chain_offset=s * a.chains)
            timed(one, a.warm)
            n1, dt1 = timed(one, a.iters)
            seq_n += n1
            seq_dt += dt1
        r = dict(sites=S, chains=S * a.chains, spec_depth=own.depth, shared_p_rate=float(np.median(rs)),
                 per_site_p_rate=float(np.median(ro)), sequential_rate=seq_n / seq_dt, shared_p_rates=rs, per_site_p_rates=ro)
        r["per_site_cost"] = 1.0 - r["per_site_p_rate"] / r["shared_p_rate"]
        r["speedup_vs_sequential"] = r["per_site_p_rate"] / r["sequential_rate"]
        print(json.dumps(r), flush=True)
        res["runs"].append(r)
    return res


def rf_coef_only(g):
    """B = 4096 models, 64 sites, each call five times with and without the table of p (kernel trace)"""
    from bayhunter_amd.synth import synth_models
    S, B = 64, 4096
    rs = np.random.RandomState(1)
    ps = spread_p(S)
    for Lmax in (10, 40):
        nlay, h, vp, vs, rho = synth_models(rs, B, Lmax, ragged=True)
        site_b = rs.randint(0, S, B)
        for joint in (False, True):
            noise = np.tile([0.0, 0.05, 0.0, 0.05, 0.5, 0.02], (B, 1))
            if not joint:
                noise = noise[:, 4:]
            for per in (False, True):
                sites = [site(g, s, ps[s] if per else 6.4) for s in range(S)]
                for jt in sites:        # exponential laws (no Gauss contraction in the trace)
                    bh.select_noise_laws(jt.targets, [True, True, False], [0.0, 0.0, 0.5])
                if not joint:
                    sites = [bh.JointTarget([jt.targets[2]]) for jt in sites]
                st = bh.SiteTargets(sites, per_site_rf=per)
                for _ in range(5):
                    st.evaluate_batch(nlay, h, vp, vs, noise, site_b, rho=rho, want_ymod=True)
    bh.default_engine(0).synchronize()


def timed(dc, iters):
    """chain-iterations/s of `iters` iterations after the burn-in start (windows as the run loop takes them)"""
    dc.engine.synchronize()
    t0 = time.perf_counter()
    start = dc.iiter
    while dc.iiter - start < iters:
        dc.iterate()
    dc.engine.synchronize()
    dt = time.perf_counter() - t0
    return dc.C * (dc.iiter - start), dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", default="1,8,64")
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warm", type=int, default=30)
    ap.add_argument("--like-only", action="store_true")
    ap.add_argument("--per-site-rf", action="store_true")
    ap.add_argument("--rf-coef-only", action="store_true")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    g = np.load(GOLDEN)
    init = dict(nchains=1, iter_burnin=5000, iter_main=100, acceptance=(40, 80), thickmin=0.1, lvz=0.1, hvz=None, rcond=None,
                maxmodels=10)
    if a.rf_coef_only:
        rf_coef_only(g)
        return
    if a.per_site_rf:
        res = per_site_rf(a, g, init)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        return
    if a.like_only:     # one evaluation batch of each path and law (exponential / Gauss on the RF), for the kernel trace
        from bayhunter_amd.synth import synth_models
        eng = bh.default_engine(0)
        S, B = 64, 4096
        rs = np.random.RandomState(1)
        nlay, h, vp, vs, rho = synth_models(rs, B, 10, ragged=True)
        noise = np.tile([0.0, 0.05, 0.0, 0.05, 0.5, 0.02], (B, 1))
        for rf_fixed, rf_corr in ((False, 0.5), (True, 0.9)):
            st = bh.SiteTargets([site(g, s) for s in range(S)])
            for s in range(S):
                bh.select_noise_laws(st.site(s).targets, [True, True, rf_fixed], [0.0, 0.0, rf_corr], rcond=1e-5)
            noise[:, 4] = rf_corr
            for _ in range(5):
                st.site(0).evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True)
                st.evaluate_batch(nlay, h, vp, vs, noise, rs.randint(0, S, B), rho=rho, want_ymod=True)
        # a long Gauss-law receiver function (n = 1024): at 4096 models the 128 x 128 contraction form (K split 2)
        from bayhunter_amd.Targets import Valuation
        n, corr = 1024, 0.9
        rinv = np.ascontiguousarray(Valuation.get_corr_inv(corr, n) / (1.0 - corr * corr))
        desc = dict(kind=bh.engine.TARGET_RF, law=bh.engine.LAW_GAUSS, n=n, nsamp=2048, p=6.4, gauss=2.5, fsamp=20.0, tshift=5.0,
                    waveno=0, rinv=rinv, logdet_r=(n - 1) * np.log(1.0 - corr * corr), yobs=np.zeros(n))
        yobs = rs.normal(0, 0.05, (S, n))
        noise1 = np.tile([corr, 0.05], (B, 1))
        for _ in range(5):
            eng.set_targets([desc])
            eng.evaluate_batch(nlay, h, vp, vs, noise1, rho=rho, want_ymod=True)
            eng.set_sites(yobs)
            eng.evaluate_sites(nlay, h, vp, vs, noise1, rs.randint(0, S, B), rho=rho, want_ymod=True)
        eng.synchronize()
        return
    res = {"chains_per_site": a.chains, "iters": a.iters, "workload": "R+L phase dispersion (21 periods) + P-RF exp law, 1..20 layers",
           "runs": []}
    for S in [int(x) for x in a.sites.split(",")]:
        st = bh.SiteTargets([site(g, s) for s in range(S)])
        dc = DeviceChains(st, a.chains, init, PRIORS, seed=5)
        timed(dc, a.warm)
        n, dt = timed(dc, a.iters)
        multi = n / dt
        seq_n, seq_dt = 0, 0.0
        for s in range(S):
            one = DeviceChains(site(g, s), a.chains, init, PRIORS, seed=5, chain_offset=s * a.chains)
            timed(one, a.warm)
            n1, dt1 = timed(one, a.iters)
            seq_n += n1
            seq_dt += dt1
        seq = seq_n / seq_dt
        r = dict(sites=S, chains=S * a.chains, spec_depth=dc.depth, sites_rate=multi, sequential_rate=seq, speedup=multi / seq,
                 sites_seconds=dt, sequential_seconds=seq_dt)
        print(json.dumps(r), flush=True)
        res["runs"].append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
