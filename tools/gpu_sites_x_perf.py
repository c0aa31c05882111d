"""Chain-iterations/s of many stations at once when every station has its own dispersion periods (SiteTargets(per_site_x=True),
include/bh_engine_sites_x.h).  The workload of tools/gpu_sites_perf.py: joint Rayleigh + Love phase dispersion + P receiver
function (exponential law), prior-like transdimensional models (1..20 layers), S sites x 8 chains.  Four runs per S:

  (a) shared_x        every site at the 21 shared periods, on the existing sites path
  (b) shared_x_table  the same sites through the period table: what the mechanism costs
  (c) own_x           sites of 15..30 periods each from different bands, in ONE DeviceChains
  (d) sequential      the sites of (c) as one-site DeviceChains runs made one after another (all a user could do before)

    python tools/gpu_sites_x_perf.py [--sites 8,64] [--iters 300] [--repeat 3] [--out profiles/sites_x_perf.json]

Each run is repeated `--repeat` times, (a), (b), (c) alternating; the best and every repeat are reported.  Only the iterations
are timed (the host-built initial states are not).

`rocprofv3 --kernel-trace --stats -- python tools/gpu_sites_x_perf.py --lean-only` gives the trial-per-lane kernel with and
without the period table on c2's shape: 4096 ten-layer models, Rayleigh + Love phase velocities at 30 periods, 64 sites that
share them, every call five times.
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


def own_periods(s):
    """site s: 15..30 periods between 1..4.5 s and 22..41 s"""
    k = 15 + (7 * s) % 16
    return np.linspace(1.0 + 0.5 * (s % 8), 22.0 + (5 * s) % 20, k)


def site(g, s, x=None):
    rs = np.random.RandomState(1000 + s)
    xs, ys = np.asarray(g["xsw"], dtype=float), np.asarray(g["ysw"], dtype=float)
    x = xs if x is None else x
    y = np.interp(x, xs, ys)
    t1 = bh.RayleighDispersionPhase(x, y + rs.normal(0, 0.02, x.size))
    t2 = bh.LoveDispersionPhase(x, 1.05 * y + rs.normal(0, 0.02, x.size))
    t3 = bh.PReceiverFunction(g["xrf"], g["yrf"] + rs.normal(0, 0.01, g["yrf"].size))
    t3.moddata.plugin.set_modelparams(gauss=1.0, p=6.4)
    return bh.JointTarget([t1, t2, t3])


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


def lean_only(g):
    from bayhunter_amd.synth import synth_models, SWD_PERIODS
    S, B = 64, 4096
    rs = np.random.RandomState(1)
    nlay, h, vp, vs, rho = synth_models(rs, B, 10, ragged=True)
    site_b = rs.randint(0, S, B)
    noise = np.tile([0.0, 0.05, 0.0, 0.05], (B, 1))
    for table in (False, True):
        sites = [bh.JointTarget(site(g, s, SWD_PERIODS).targets[:2]) for s in range(S)]
        for jt in sites:
            for t in jt.targets:
                t.set_noise_law("nocorr")
        st = bh.SiteTargets(sites, per_site_x=table)
        for _ in range(5):
            st.evaluate_batch(nlay, h, vp, vs, noise, site_b, rho=rho)
        print("period table %s: kernel %s" % (table, st.engine.last_swd_kernel()), flush=True)
    bh.default_engine(0).synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", default="8,64")
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warm", type=int, default=30)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--lean-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    g = np.load(GOLDEN)
    if a.lean_only:
        lean_only(g)
        return
    init = dict(nchains=1, iter_burnin=5000, iter_main=100, acceptance=(40, 80), thickmin=0.1, lvz=0.1, hvz=None, rcond=None,
                maxmodels=10)
    res = {"chains_per_site": a.chains, "iters": a.iters, "repeat": a.repeat,
           "workload": "R+L phase dispersion + P-RF exp law, 1..20 layers; shared: 21 periods, own: 15..30 periods per site", "runs": []}
    for S in [int(x) for x in a.sites.split(",")]:
        xs = [own_periods(s) for s in range(S)]
        runs = {"shared_x": DeviceChains(bh.SiteTargets([site(g, s) for s in range(S)]), a.chains, init, PRIORS, seed=5),
                "shared_x_table": DeviceChains(bh.SiteTargets([site(g, s) for s in range(S)], per_site_x=True), a.chains, init, PRIORS, seed=5),
                "own_x": DeviceChains(bh.SiteTargets([site(g, s, xs[s]) for s in range(S)], per_site_x=True), a.chains, init, PRIORS, seed=5)}
        rates = {k: [] for k in runs}
        for dc in runs.values():
            timed(dc, a.warm)
        for _ in range(a.repeat):       # alternating: drifts of the clock or the host hit all alike
            for k, dc in runs.items():
                timed(dc, 5)            # (the engine's registration changes hands: outside the timed part, as for (d))
                n, dt = timed(dc, a.iters)
                rates[k].append(n / dt)
        seq = []
        ones = []
        for s in range(S):
            one = DeviceChains(site(g, s, xs[s]), a.chains, init, PRIORS, seed=5, chain_offset=s * a.chains)
            timed(one, a.warm)
            ones.append(one)
        for _ in range(a.repeat):
            seq_n, seq_dt = 0, 0.0
            for one in ones:
                timed(one, 5)
                n1, dt1 = timed(one, a.iters)
                seq_n += n1
                seq_dt += dt1
            seq.append(seq_n / seq_dt)
        r = dict(sites=S, chains=S * a.chains, spec_depth=runs["own_x"].depth, periods_per_site=[int(x.size) for x in xs],
                 shared_x_rate=max(rates["shared_x"]), shared_x_table_rate=max(rates["shared_x_table"]), own_x_rate=max(rates["own_x"]),
                 sequential_rate=max(seq), shared_x_rates=rates["shared_x"], shared_x_table_rates=rates["shared_x_table"],
                 own_x_rates=rates["own_x"], sequential_rates=seq)
        r["table_cost"] = 1.0 - r["shared_x_table_rate"] / r["shared_x_rate"]
        r["speedup_vs_sequential"] = r["own_x_rate"] / r["sequential_rate"]
        r["sequential_spread"] = (max(seq) - min(seq)) / max(seq)
        print(json.dumps(r), flush=True)
        res["runs"].append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
