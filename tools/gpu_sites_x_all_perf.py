"""Chain-iterations/s of many stations at once when every station has its own periods on its phase AND group-velocity curves
(SiteTargets(per_site_x="all"), include/bh_engine_sites_x_all.h), and the launch of second roots with and without the table.
Workload: Rayleigh phase + Rayleigh group dispersion + P receiver function (exponential law), prior-like transdimensional
models (1..20 layers), S sites x 8 chains.  Four runs per S:

  (a) shared_x        every site at the 21 shared periods on both curves, on the shared-x sites path (as before this option)
      shared_x_table  the same sites through the period table of per_site_x="all": what the mechanism costs
  (b) own_x           sites of 15..30 periods on each curve, from different bands, in ONE DeviceChains
      sequential      the sites of own_x as one-site DeviceChains runs made one after another

    python tools/gpu_sites_x_all_perf.py [--sites 8,64] [--iters 300] [--repeat 3] [--out profiles/sites_x_all_perf.json]

Each run is repeated `--repeat` times, shared_x, shared_x_table and own_x alternating; the best and every repeat are reported.
Only the iterations are timed.

  (c) `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/gpu_sites_x_all_perf.py --second MODE`
gives the kernel time of the launch of second roots at c2g's shape -- 4096 ten-layer models, Rayleigh + Love group velocities
at 30 periods, 64 sites, every call five times -- MODE = shared (the plain site table: swd_kernel(SwdKernelArgs)), table (the same
periods through the table: swd_kernel(SwdKernelArgs, SwdSiteXArgs)) or spread (15..30 periods per site: the share of idle
entries is printed).  `--second-stats shared=CSV,table=CSV,spread=CSV --out FILE` puts the swd_kernel rows of the three
kernel_stats files into FILE's "second_roots".
"""
import argparse
import csv
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
    """15..30 periods between 1..4.5 s and 22..41 s"""
    k = 15 + (7 * s) % 16
    return np.linspace(1.0 + 0.5 * (s % 8), 22.0 + (5 * s) % 20, k)


def site(g, s, xp=None, xg=None):
    rs = np.random.RandomState(1000 + s)
    xs, ys = np.asarray(g["xsw"], dtype=float), np.asarray(g["ysw"], dtype=float)
    xp, xg = xs if xp is None else xp, xs if xg is None else xg
    t1 = bh.RayleighDispersionPhase(xp, np.interp(xp, xs, ys) + rs.normal(0, 0.02, xp.size))
    t2 = bh.RayleighDispersionGroup(xg, 0.9 * np.interp(xg, xs, ys) + rs.normal(0, 0.02, xg.size))
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


def second_only(mode):
    from bayhunter_amd.synth import synth_models, SWD_PERIODS
    S, B = 64, 4096
    rs = np.random.RandomState(1)
    nlay, h, vp, vs, rho = synth_models(rs, B, 10, ragged=True)
    site_b = rs.randint(0, S, B)
    noise = np.tile([0.0, 0.05, 0.0, 0.05], (B, 1))
    per = np.asarray(SWD_PERIODS, dtype=float)
    counts = [per.size if mode != "spread" else 15 + (7 * s) % 16 for s in range(S)]
    sites = []
    for s in range(S):
        x = per[:counts[s]]
        ts = [bh.RayleighDispersionGroup(x, 3.0 + 0.01 * x), bh.LoveDispersionGroup(x, 3.3 + 0.01 * x)]
        for t in ts:
            t.set_noise_law("nocorr")
        sites.append(bh.JointTarget(ts))
    st = bh.SiteTargets(sites, per_site_x=False if mode == "shared" else "all")
    for _ in range(5):
        st.evaluate_batch(nlay, h, vp, vs, noise, site_b, rho=rho)
    cap = max(counts)
    idle = 1.0 - float(np.mean(np.asarray(counts)[site_b])) / cap
    print(json.dumps(dict(mode=mode, capacity=cap, entries_per_target=B * cap, idle_share=idle,
                          launches=[(l["family"], l["role"]) for l in st.engine.last_swd_launches()])), flush=True)
    bh.default_engine(0).synchronize()


def second_stats(spec, out):
    res = {}
    if out and os.path.exists(out):
        with open(out) as f:
            res = json.load(f)
    rows = {}
    for item in spec.split(","):
        mode, path = item.split("=", 1)
        with open(path) as f:
            for r in csv.DictReader(f):
                if "swd_kernel<" in r["Name"]:
                    rows.setdefault(mode, []).append(dict(kernel=r["Name"], calls=int(r["Calls"]), avg_us=float(r["AverageNs"]) / 1e3,
                                                          min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3))
    res["second_roots"] = dict(shape="B = 4096 ragged ten-layer models, Rayleigh + Love group velocities, 30 periods (capacity), 64 sites, "
                                     "reference sequence, every call five times; duration per dispatch", modes=rows)
    print(json.dumps(res["second_roots"]), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", default="8,64")
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warm", type=int, default=30)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--second", choices=["shared", "table", "spread"], default=None)
    ap.add_argument("--second-stats", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.second_stats:
        second_stats(a.second_stats, a.out)
        return
    if a.second:
        second_only(a.second)
        return
    g = np.load(GOLDEN)
    init = dict(nchains=1, iter_burnin=5000, iter_main=100, acceptance=(40, 80), thickmin=0.1, lvz=0.1, hvz=None, rcond=None,
                maxmodels=10)
    res = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res.update({"chains_per_site": a.chains, "iters": a.iters, "repeat": a.repeat,
                "workload": "R phase + R group dispersion + P-RF exp law, 1..20 layers; shared: 21 periods on both curves, "
                            "own: 15..30 periods per site and curve", "runs": []})
    for S in [int(x) for x in a.sites.split(",")]:
        xp, xg = [own_periods(s) for s in range(S)], [own_periods(s + 3) for s in range(S)]
        runs = {"shared_x": DeviceChains(bh.SiteTargets([site(g, s) for s in range(S)]), a.chains, init, PRIORS, seed=5),
                "shared_x_table": DeviceChains(bh.SiteTargets([site(g, s) for s in range(S)], per_site_x="all"), a.chains, init, PRIORS, seed=5),
                "own_x": DeviceChains(bh.SiteTargets([site(g, s, xp[s], xg[s]) for s in range(S)], per_site_x="all"), a.chains, init, PRIORS, seed=5)}
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
            one = DeviceChains(site(g, s, xp[s], xg[s]), a.chains, init, PRIORS, seed=5, chain_offset=s * a.chains)
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
        r = dict(sites=S, chains=S * a.chains, spec_depth=runs["own_x"].depth,
                 periods_per_site=[[int(x.size), int(y.size)] for x, y in zip(xp, xg)],
                 shared_x_rate=max(rates["shared_x"]), shared_x_table_rate=max(rates["shared_x_table"]), own_x_rate=max(rates["own_x"]),
                 sequential_rate=max(seq), shared_x_rates=rates["shared_x"], shared_x_table_rates=rates["shared_x_table"],
                 own_x_rates=rates["own_x"], sequential_rates=seq)
        r["table_cost"] = 1.0 - r["shared_x_table_rate"] / r["shared_x_rate"]
        r["shared_x_spread"] = spread(rates["shared_x"])
        r["shared_x_table_spread"] = spread(rates["shared_x_table"])
        r["table_within_shared_x_spread"] = bool(r["shared_x_table_rate"] >= min(rates["shared_x"]))
        r["speedup_vs_sequential"] = r["own_x_rate"] / r["sequential_rate"]
        r["own_x_spread"] = spread(rates["own_x"])
        r["sequential_spread"] = spread(seq)
        print(json.dumps(r), flush=True)
        res["runs"].append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
