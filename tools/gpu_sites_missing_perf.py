"""Chain-iterations/s of many stations at once when stations LACK some of the array's targets (SiteTargets(missing=True),
include/bh_engine_sites_missing.h), and whether what a station lacks is skipped or computed and ignored.
Workload: Rayleigh phase + Rayleigh group dispersion + P receiver function (exponential law), prior-like transdimensional
models (1..20 layers), S sites x 8 chains, every site 15..30 periods of its own on each curve.  Per S:

  (a) all_x        every site has every slot, through SiteTargets(per_site_x="all") -- the path as it was
      all_missing  the same sites through SiteTargets(missing=True): what the mechanism costs
  (b) lacking      every second site without the receiver function, every fourth without the group curve, in ONE DeviceChains
      sequential   the sites of `lacking` as one-site DeviceChains runs over the targets each has, made one after another

    python tools/gpu_sites_missing_perf.py [--sites 8,64] [--iters 300] [--repeat 3] [--out profiles/sites_missing_perf.json]

Each run is repeated `--repeat` times, all_x, all_missing and lacking alternating; the best and every repeat are reported.
Only the iterations are timed.

  (c) `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/gpu_sites_missing_perf.py --trace MODE`
runs five evaluate calls of 4096 ten-layer models over 64 sites through SiteTargets(missing=True): MODE rf_all / rf_half --
Rayleigh phase + P receiver function, every site / every second site with the receiver function (the synthesis kernel's time);
gr_all / gr_quarter -- Rayleigh phase + Rayleigh group velocities, every site / three of four with the group curve (the launch of
second roots).  `--trace-stats rf_all=CSV,rf_half=CSV,gr_all=CSV,gr_quarter=CSV --out FILE` puts the rows of the synthesis kernel
and of the second-root launch into FILE's "skipped".
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


def lacks(s):
    """(no receiver function, no group curve) of site s: every second site, every fourth"""
    return s % 2 == 1, s % 4 == 2


def slots(g, s, everything=False):
    """[Rayleigh phase, Rayleigh group, P receiver function] of site s, None where it lacks the slot"""
    rs = np.random.RandomState(1000 + s)
    xs, ys = np.asarray(g["xsw"], dtype=float), np.asarray(g["ysw"], dtype=float)
    xp, xg = own_periods(s), own_periods(s + 3)
    t1 = bh.RayleighDispersionPhase(xp, np.interp(xp, xs, ys) + rs.normal(0, 0.02, xp.size))
    t2 = bh.RayleighDispersionGroup(xg, 0.9 * np.interp(xg, xs, ys) + rs.normal(0, 0.02, xg.size))
    t3 = bh.PReceiverFunction(g["xrf"], g["yrf"] + rs.normal(0, 0.01, g["yrf"].size))
    t3.moddata.plugin.set_modelparams(gauss=1.0, p=6.4)
    no_rf, no_gr = (False, False) if everything else lacks(s)
    return [t1, None if no_gr else t2, None if no_rf else t3]


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


def trace_only(mode):
    from bayhunter_amd.synth import synth_models, SWD_PERIODS
    g = np.load(GOLDEN)
    S, B = 64, 4096
    rs = np.random.RandomState(1)
    nlay, h, vp, vs, rho = synth_models(rs, B, 10, ragged=True)
    site_b = rs.randint(0, S, B)
    per = np.asarray(SWD_PERIODS, dtype=float)
    rows = []
    for s in range(S):
        t1 = bh.RayleighDispersionPhase(per, 3.0 + 0.01 * per)
        t1.set_noise_law("nocorr")
        if mode.startswith("rf"):
            t2 = bh.PReceiverFunction(g["xrf"], g["yrf"])
            t2.moddata.plugin.set_modelparams(gauss=1.0, p=6.4)
            t2.set_noise_law("exp")
            gone = mode == "rf_half" and s % 2 == 1
        else:
            t2 = bh.RayleighDispersionGroup(per, 2.8 + 0.01 * per)
            t2.set_noise_law("nocorr")
            gone = mode == "gr_quarter" and s % 4 == 2
        rows.append([t1, None if gone else t2])
    st = bh.SiteTargets(rows, per_site_x="all", missing=True)
    st.engine.set_swd_search("reference")
    noise = np.tile([0.0, 0.05, 0.5 if mode.startswith("rf") else 0.0, 0.05], (B, 1))
    for _ in range(5):
        st.evaluate_batch(nlay, h, vp, vs, noise, site_b, rho=rho)
    share = float(np.mean(~st.present[site_b, 1]))
    print(json.dumps(dict(mode=mode, models=B, sites=S, share_of_models_without_the_slot=share,
                          launches=[(l["family"], l["role"]) for l in st.engine.last_swd_launches()])), flush=True)
    st.engine.synchronize()


def trace_stats(spec, out):
    res = {}
    if out and os.path.exists(out):
        with open(out) as f:
            res = json.load(f)
    rows = {}
    for item in spec.split(","):
        mode, path = item.split("=", 1)
        want = "rf_synth" if mode.startswith("rf") else "swd_kernel<"
        with open(path) as f:
            for r in csv.DictReader(f):
                if want in r["Name"]:
                    rows.setdefault(mode, []).append(dict(kernel=r["Name"], calls=int(r["Calls"]), avg_us=float(r["AverageNs"]) / 1e3,
                                                          min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3))
    res["skipped"] = dict(shape="B = 4096 ragged ten-layer models over 64 sites through SiteTargets(missing=True), reference sequence, "
                                "every call five times; duration per dispatch.  rf_*: the synthesis kernel, every site / every "
                                "second site with the receiver function; gr_*: the launch of second roots, every site / three of "
                                "four with the group curve", modes=rows)
    avg = lambda m: sum(r["avg_us"] * r["calls"] for r in rows.get(m, [])) / max(1, sum(r["calls"] for r in rows.get(m, [])))
    if "rf_all" in rows and "rf_half" in rows:
        res["skipped"]["rf_half_over_all"] = avg("rf_half") / avg("rf_all")
    if "gr_all" in rows and "gr_quarter" in rows:
        res["skipped"]["gr_quarter_over_all"] = avg("gr_quarter") / avg("gr_all")
    print(json.dumps(res["skipped"]), flush=True)
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
    ap.add_argument("--trace", choices=["rf_all", "rf_half", "gr_all", "gr_quarter"], default=None)
    ap.add_argument("--trace-stats", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace_stats:
        trace_stats(a.trace_stats, a.out)
        return
    if a.trace:
        trace_only(a.trace)
        return
    g = np.load(GOLDEN)
    init = dict(nchains=1, iter_burnin=5000, iter_main=100, acceptance=(40, 80), thickmin=0.1, lvz=0.1, hvz=None, rcond=None,
                maxmodels=10)
    res = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res.update({"chains_per_site": a.chains, "iters": a.iters, "repeat": a.repeat,
                "workload": "R phase + R group dispersion + P-RF exp law, 1..20 layers, 15..30 periods per site and curve; lacking: "
                            "every second site without the receiver function, every fourth without the group curve", "runs": []})
    for S in [int(x) for x in a.sites.split(",")]:
        M = dict(per_site_x="all", per_site_rf=True)
        runs = {"all_x": DeviceChains(bh.SiteTargets([bh.JointTarget(slots(g, s, True)) for s in range(S)], **M), a.chains, init, PRIORS, seed=5),
                "all_missing": DeviceChains(bh.SiteTargets([slots(g, s, True) for s in range(S)], missing=True, **M), a.chains, init, PRIORS, seed=5),
                "lacking": DeviceChains(bh.SiteTargets([slots(g, s) for s in range(S)], missing=True, **M), a.chains, init, PRIORS, seed=5)}
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
            own = bh.JointTarget([t for t in slots(g, s) if t is not None])
            one = DeviceChains(own, a.chains, init, PRIORS, seed=5, chain_offset=s * a.chains)
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
        r = dict(sites=S, chains=S * a.chains, spec_depth=runs["lacking"].depth,
                 sites_without_rf=int(sum(lacks(s)[0] for s in range(S))), sites_without_group=int(sum(lacks(s)[1] for s in range(S))),
                 all_x_rate=max(rates["all_x"]), all_missing_rate=max(rates["all_missing"]), lacking_rate=max(rates["lacking"]),
                 sequential_rate=max(seq), all_x_rates=rates["all_x"], all_missing_rates=rates["all_missing"],
                 lacking_rates=rates["lacking"], sequential_rates=seq)
        r["mechanism_cost"] = 1.0 - r["all_missing_rate"] / r["all_x_rate"]
        r["all_x_spread"] = spread(rates["all_x"])
        r["all_missing_spread"] = spread(rates["all_missing"])
        r["missing_within_all_x_spread"] = bool(r["all_missing_rate"] >= min(rates["all_x"]))
        r["speedup_vs_sequential"] = r["lacking_rate"] / r["sequential_rate"]
        r["lacking_spread"] = spread(rates["lacking"])
        r["sequential_spread"] = spread(seq)
        print(json.dumps(r), flush=True)
        res["runs"].append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
