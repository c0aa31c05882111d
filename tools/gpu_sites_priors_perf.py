"""Chain-iterations/s of many stations at once when every station carries its OWN priors and sampler settings (DeviceChains with
one dict per site, include/bh_engine_sites_priors.h).
Workload: Rayleigh phase + Rayleigh group dispersion + P receiver function (exponential law), S sites x 8 chains, every site
15..30 periods of its own on each curve.  Per S:

  (a) shared       every site under one dict of priors, through the chain calls without a table -- the path as it was
      table        the same run with prior_table=True: every chain reads its site's (equal) record -- what the mechanism costs
  (b) own          sites with different priors (layer and velocity ranges, noise ranges, a fixed vp/vs or the mantle rule at some,
                   thickmin / lvz / hvz, acceptance bands, proposal widths) in ONE DeviceChains
      sequential   the sites of `own` as one-site DeviceChains runs with their own dicts, made one after another

    python tools/gpu_sites_priors_perf.py [--sites 8,64] [--iters 300] [--repeat 3] [--out profiles/sites_priors_perf.json]

Each run is repeated `--repeat` times, shared, table and own alternating; the best and every repeat are reported.  Only the
iterations are timed.
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
INIT = dict(nchains=1, iter_burnin=5000, iter_main=100, acceptance=(40, 80), thickmin=0.1, lvz=0.1, hvz=None, rcond=None,
            maxmodels=10)
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "chain_golden.npz")


def own_periods(s):
    """15..30 periods between 1..4.5 s and 22..41 s"""
    k = 15 + (7 * s) % 16
    return np.linspace(1.0 + 0.5 * (s % 8), 22.0 + (5 * s) % 20, k)


def targets(g, s):
    """[Rayleigh phase, Rayleigh group, P receiver function] of site s"""
    rs = np.random.RandomState(1000 + s)
    xs, ys = np.asarray(g["xsw"], dtype=float), np.asarray(g["ysw"], dtype=float)
    xp, xg = own_periods(s), own_periods(s + 3)
    t1 = bh.RayleighDispersionPhase(xp, np.interp(xp, xs, ys) + rs.normal(0, 0.02, xp.size))
    t2 = bh.RayleighDispersionGroup(xg, 0.9 * np.interp(xg, xs, ys) + rs.normal(0, 0.02, xg.size))
    t3 = bh.PReceiverFunction(g["xrf"], g["yrf"] + rs.normal(0, 0.01, g["yrf"].size))
    t3.moddata.plugin.set_modelparams(gauss=1.0, p=6.4)
    return bh.JointTarget([t1, t2, t3])


def own_dicts(s):
    """(initparams, modelpriors) of site s: four kinds of station, with a Moho estimate and noise ranges of its own"""
    pr = dict(PRIORS, mohoest=(30.0 + s % 11, 3.0), rfnoise_sigma=(1e-5, 0.03 + 0.002 * (s % 10)),
              swdnoise_sigma=(1e-5, 0.06 + 0.004 * (s % 10)))
    ip = dict(INIT, acceptance=(35 + s % 10, 75 + s % 10))
    kind = s % 4
    if kind == 1:      # a basin station: slow, thin layers allowed, fewer of them
        pr.update(vs=(1.5, 4.5), z=(0, 50), layers=(1, 12))
        ip.update(thickmin=0.05, lvz=0.2, propdist=(0.03, 0.03, 0.02, 0.005, 0.005))
    elif kind == 2:    # a craton station: fast, fixed vp/vs, no velocity inversions
        pr.update(vs=(2.5, 5), vpvs=1.73, layers=(2, 16))
        ip.update(thickmin=0.5, lvz=None, hvz=0.5)
    elif kind == 3:    # the mantle rule
        pr.update(mantle=(4.2, 1.8), z=(0, 70))
    return ip, pr


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
    ap.add_argument("--sites", default="8,64")
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warm", type=int, default=30)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    g = np.load(GOLDEN)
    res = {"chains_per_site": a.chains, "iters": a.iters, "repeat": a.repeat,
           "workload": "R phase + R group dispersion + P-RF exp law, 15..30 periods per site and curve; shared / table: every site "
                       "under one dict of priors (1..20 layers), without / with the table of records; own: four kinds of station "
                       "(layers 20 / 12 / 16 / 20 at most, vs and z ranges, fixed vp/vs, mantle rule, thickmin, lvz / hvz, proposal "
                       "widths) with a Moho estimate, noise ranges and an acceptance band per site", "runs": []}
    for S in [int(x) for x in a.sites.split(",")]:
        M = dict(per_site_x="all", per_site_rf=True)
        mk = lambda: bh.SiteTargets([targets(g, s) for s in range(S)], **M)
        dicts = [own_dicts(s) for s in range(S)]
        runs = {"shared": DeviceChains(mk(), a.chains, INIT, PRIORS, seed=5),
                "table": DeviceChains(mk(), a.chains, INIT, PRIORS, seed=5, prior_table=True),
                "own": DeviceChains(mk(), a.chains, [d[0] for d in dicts], [d[1] for d in dicts], seed=5)}
        assert not runs["shared"].prior_table and runs["table"].prior_table and runs["own"].prior_table
        rates = {k: [] for k in runs}
        for dc in runs.values():
            timed(dc, a.warm)
        for _ in range(a.repeat):       # alternating: drifts of the clock or the host hit all alike
            for k, dc in runs.items():
                timed(dc, 5)            # (the engine's registration changes hands: outside the timed part, as for `sequential`)
                n, dt = timed(dc, a.iters)
                rates[k].append(n / dt)
        print("[%d sites] runs in one DeviceChains done" % S, file=sys.stderr, flush=True)
        seq, ones = [], []
        for s in range(S):
            one = DeviceChains(targets(g, s), a.chains, dicts[s][0], dicts[s][1], seed=5, chain_offset=s * a.chains)
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
            print("[%d sites] one-site runs, repeat %d done" % (S, len(seq)), file=sys.stderr, flush=True)
        spread = lambda v: (max(v) - min(v)) / max(v)
        r = dict(sites=S, chains=S * a.chains, spec_depth=runs["own"].depth, one_site_spec_depth=ones[0].depth,
                 shared_rate=max(rates["shared"]), table_rate=max(rates["table"]), own_rate=max(rates["own"]),
                 sequential_rate=max(seq), shared_rates=rates["shared"], table_rates=rates["table"], own_rates=rates["own"],
                 sequential_rates=seq)
        r["mechanism_cost"] = 1.0 - r["table_rate"] / r["shared_rate"]
        r["shared_spread"] = spread(rates["shared"])
        r["table_spread"] = spread(rates["table"])
        r["table_within_shared_spread"] = bool(r["table_rate"] >= min(rates["shared"]))
        r["speedup_vs_sequential"] = r["own_rate"] / r["sequential_rate"]
        r["own_spread"] = spread(rates["own"])
        r["sequential_spread"] = spread(seq)
        print(json.dumps(r), flush=True)
        res["runs"].append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
