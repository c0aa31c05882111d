"""What a receiver-function time axis and Gauss filter per site cost (SiteTargets(per_site_rf="all"),
include/bh_engine_sites_rf_axis.h), and chain-iterations/s of stations processed with different windows, sampling and filters.

  (a) the mechanism, kernels: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python
      tools/gpu_sites_rf_axis_perf.py --trace MODE`, a run per MODE, makes evaluate calls of 4096 ten-layer models over 64 sites on
      one P receiver function (exponential law):
        mechanism    sites that all share ONE axis (2048 / 1000 samples / 20 Hz / 2.5): five calls on the existing missing=True path
                     (rf_synth_m_kernel: the yardstick, with its own call-to-call range) alternating with five through the axis
                     table (rf_synth_t_kernel)
        mix_512 / mix_8192 / mix_both
                     every site at nsamp 512 (201 samples, 5 Hz), every site at 8192 (4000 samples, 20 Hz), and the sites
                     alternating between the two: every workgroup of the last holds the long trace's LDS
      `--trace-stats MODE=CSV,... --out FILE` puts the rows of the synthesis kernels into FILE's "kernels".
  (b) the mechanism, chains: Rayleigh phase + P receiver function, S sites x 8 chains that all share one axis:
        table        SiteTargets(per_site_x="all", per_site_rf="all")
        shared       SiteTargets(per_site_x="all", per_site_rf=True, missing=True): the existing path
  (c) the use case: the same stations with four different axes and filter widths (AXES) in ONE DeviceChains against the one-site
      runs made one after another.

    python tools/gpu_sites_rf_axis_perf.py [--sites 8,64] [--iters 300] [--repeat 3] [--out profiles/sites_rf_axis_perf.json]

Each run is repeated `--repeat` times, the two sides alternating; the best and every repeat are reported.  Only the iterations are
timed.
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
from bayhunter_amd import engine as E  # noqa: E402
from bayhunter_amd.device_chains import DeviceChains  # noqa: E402

PRIORS = dict(vpvs=(1.4, 2.1), layers=(1, 20), vs=(2, 5), z=(0, 60), rfnoise_corr=(0.35, 0.75),
              rfnoise_sigma=(1e-5, 0.05), swdnoise_corr=0., swdnoise_sigma=(1e-5, 0.1))
INIT = dict(nchains=1, iter_burnin=5000, iter_main=100, acceptance=(40, 80), thickmin=0.1, lvz=0.1, hvz=None, rcond=1e-5,
            maxmodels=10)
# (samples, rate Hz, shift s, gauss): windows of -5 .. 35 s at 5 Hz, -5 .. 20 s at 10 Hz, -10 .. 40 s at 20 Hz, -2 .. 23 s at 4 Hz;
# transforms of 512, 512, 2048 and 256 points
AXES = [(201, 5.0, 5.0, 2.5), (250, 10.0, 5.0, 1.0), (1000, 20.0, 10.0, 2.5), (100, 4.0, 2.0, 1.0)]
TRACE_MODES = ["mechanism", "mix_512", "mix_8192", "mix_both"]
KERNELS = ("rf_synth", "rf_coef")


def station(s, axis):
    """[Rayleigh phase, P receiver function on `axis`] of site s"""
    rs = np.random.RandomState(1000 + s)
    per = np.linspace(2.0 + 0.25 * (s % 8), 40.0 + (3 * s) % 15, 15 + (7 * s) % 16)
    t1 = bh.RayleighDispersionPhase(per, 3.2 + 0.015 * per + rs.normal(0, 0.02, per.size))
    n, fsamp, tshift, gauss = axis
    x = np.arange(n) / fsamp - tshift
    t2 = bh.PReceiverFunction(x, 0.4 * np.exp(-(x / 0.6) ** 2) + 0.1 * np.exp(-((x - 4.0) / 0.8) ** 2) + rs.normal(0, 0.01, n))
    t2.moddata.plugin.set_modelparams(gauss=gauss, p=5.0 + 0.05 * (s % 60))
    return [t1, t2]


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


def axis_tables(S, nt, axes_of):
    nsamp = np.full((S, nt), 4, np.int32)
    fsamp, tshift, gauss = np.ones((S, nt)), np.zeros((S, nt)), np.ones((S, nt))
    for s in range(S):
        nsamp[s, 0], _, fsamp[s, 0], tshift[s, 0], gauss[s, 0] = axes_of(s)
    return nsamp, fsamp, tshift, gauss


def trace_only(mode):
    from bayhunter_amd.synth import synth_models
    S, B = 64, 4096
    rs = np.random.RandomState(1)
    nlay, h, vp, vs, rho = synth_models(rs, B, 10, ragged=True)
    site = rs.randint(0, S, B).astype(np.int32)
    noise = np.tile([0.5, 0.05], (B, 1))
    short, mid, long_ = (512, 201, 5.0, 5.0, 2.5), (2048, 1000, 20.0, 5.0, 2.5), (8192, 4000, 20.0, 5.0, 2.5)
    axes_of = {"mechanism": lambda s: mid, "mix_512": lambda s: short, "mix_8192": lambda s: long_,
               "mix_both": lambda s: long_ if s % 2 else short}[mode]
    cap, nmax = max(axes_of(s)[1] for s in range(S)), max(axes_of(s)[0] for s in range(S))
    n = np.array([[axes_of(s)[1]] for s in range(S)], np.int32)
    yobs = rs.normal(0, 0.05, (S, cap))
    for s in range(S):
        yobs[s, n[s, 0]:] = 0.0
    p, nsv = np.full((S, 1), 6.4), np.zeros((S, 1))
    a0 = axes_of(0)
    desc = dict(kind=E.TARGET_RF, law=E.LAW_EXP, n=cap, waveno=0, p=6.4, gauss=a0[4], tshift=a0[3], nsamp=nmax, fsamp=a0[2], yobs=np.zeros(cap))
    eng = E.default_engine(0)
    eng.set_targets([desc])
    for rep in range(5):
        if mode == "mechanism":         # the existing path of sites that may lack targets: rf_synth_m_kernel
            eng.set_sites_missing(n, np.zeros((S, cap)), yobs)
            eng.set_sites_rf(p, nsv)
            eng.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho)
        eng.set_sites_axes(n, np.zeros((S, cap)), yobs)
        eng.set_sites_rf(p, nsv)
        eng.set_sites_rf_axis(*axis_tables(S, 1, axes_of))
        eng.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho)
    eng.synchronize()
    print(json.dumps(dict(mode=mode, models=B, sites=S, capacity=int(cap), nsamp_max=int(nmax))), flush=True)


def trace_stats(spec, out):
    res = {}
    if out and os.path.exists(out):
        with open(out) as f:
            res = json.load(f)
    rows = {}
    for item in spec.split(","):
        mode, path = item.split("=", 1)
        with open(path) as f:
            for r in csv.DictReader(f):
                if any(k in r["Name"] for k in KERNELS):
                    rows.setdefault(mode, []).append(dict(kernel=r["Name"], calls=int(r["Calls"]), avg_us=float(r["AverageNs"]) / 1e3,
                                                          min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3))
    res["kernels"] = dict(shape="B = 4096 ragged ten-layer models over 64 sites, one P receiver function, exponential law, five calls; "
                                "duration per dispatch.  mechanism: every site at 2048 / 1000 samples / 20 Hz / 2.5, the missing=True "
                                "path (rf_synth_m_kernel) alternating with the axis table (rf_synth_t_kernel); mix_*: every site at nsamp "
                                "512, every site at 8192, the sites alternating between the two", modes=rows)

    def synth(mode, name):
        r = [x for x in rows.get(mode, []) if name in x["kernel"]]
        return r[0] if r else None
    m, t = synth("mechanism", "rf_synth_m_kernel"), synth("mechanism", "rf_synth_t_kernel")
    if m and t:
        res["kernels"]["mechanism_summary"] = dict(parent_avg_us=m["avg_us"], parent_range_us=[m["min_us"], m["max_us"]],
                                                   table_avg_us=t["avg_us"], table_range_us=[t["min_us"], t["max_us"]],
                                                   table_over_parent=t["avg_us"] / m["avg_us"])
    mix = {k: synth("mix_" + k, "rf_synth_t_kernel") for k in ("512", "8192", "both")}
    if all(mix.values()):
        separate = 0.5 * (mix["512"]["avg_us"] + mix["8192"]["avg_us"])
        res["kernels"]["mix_summary"] = dict(all_512_us=mix["512"]["avg_us"], all_8192_us=mix["8192"]["avg_us"], mixed_us=mix["both"]["avg_us"],
                                             half_of_each_us=separate, mixed_over_half_of_each=mix["both"]["avg_us"] / separate)
    print(json.dumps({k: v for k, v in res["kernels"].items() if k.endswith("summary")}), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


def race(a_side, b_sides, warm, iters, repeat, tag):
    """a_side (one DeviceChains) against b_sides (one or many, run one after another), alternating; rates of every repeat"""
    timed(a_side, warm)
    for b in b_sides:
        b.targets._register()     # (a run registers its targets when it is made: the engine has changed hands since)
        timed(b, warm)
    ar, br = [], []
    for _ in range(repeat):       # alternating: drifts of the clock or the host hit both alike
        timed(a_side, 5)          # (the run takes the engine's registration back: outside the timed part)
        n, dt = timed(a_side, iters)
        ar.append(n / dt)
        bn, bdt = 0, 0.0
        for b in b_sides:
            b.targets._register()
            timed(b, 5)
            n1, dt1 = timed(b, iters)
            bn += n1
            bdt += dt1
        br.append(bn / bdt)
        print("[%s] repeat %d done" % (tag, len(br)), file=sys.stderr, flush=True)
    return ar, br


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", default="8,64")
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warm", type=int, default=30)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--trace", choices=TRACE_MODES, default=None)
    ap.add_argument("--trace-stats", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace_stats:
        trace_stats(a.trace_stats, a.out)
        return
    if a.trace:
        trace_only(a.trace)
        return
    res = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res.update({"chains_per_site": a.chains, "iters": a.iters, "repeat": a.repeat,
                "workload": "R phase dispersion (15..30 periods per site) + P-RF, exponential law, 1..20 layers.  mechanism: every site "
                            "on the axis 201 samples / 5 Hz / 2.5; use_case: the sites on four axes in turn -- 201 / 5 Hz / 2.5, 250 / "
                            "10 Hz / 1.0, 1000 / 20 Hz / 2.5, 100 / 4 Hz / 1.0 (samples / rate / gauss)", "mechanism": [], "use_case": []})
    spread = lambda v: (max(v) - min(v)) / max(v)
    for S in [int(x) for x in a.sites.split(",")]:
        same = [station(s, AXES[0]) for s in range(S)]
        table = DeviceChains(bh.SiteTargets(same, per_site_x="all", per_site_rf="all"), a.chains, INIT, PRIORS, seed=5)
        shared = DeviceChains(bh.SiteTargets(same, per_site_x="all", per_site_rf=True, missing=True), a.chains, INIT, PRIORS, seed=5)
        tr, sr = race(table, [shared], a.warm, a.iters, a.repeat, "%d sites, mechanism" % S)
        r = dict(sites=S, chains=S * a.chains, spec_depth=table.depth, table_rate=max(tr), shared_rate=max(sr), table_rates=tr,
                 shared_rates=sr, table_spread=spread(tr), shared_spread=spread(sr), table_over_shared=max(tr) / max(sr))
        print(json.dumps(r), flush=True)
        res["mechanism"].append(r)
        del table, shared
        mixed = [station(s, AXES[s % len(AXES)]) for s in range(S)]
        own = DeviceChains(bh.SiteTargets(mixed, per_site_x="all", per_site_rf="all"), a.chains, INIT, PRIORS, seed=5)
        ones = [DeviceChains(bh.JointTarget(mixed[s]), a.chains, INIT, PRIORS, seed=5, chain_offset=s * a.chains) for s in range(S)]
        orr, seq = race(own, ones, a.warm, a.iters, a.repeat, "%d sites, use case" % S)
        r = dict(sites=S, chains=S * a.chains, spec_depth=own.depth, one_site_spec_depth=ones[0].depth, own_rate=max(orr),
                 sequential_rate=max(seq), own_rates=orr, sequential_rates=seq, own_spread=spread(orr), sequential_spread=spread(seq),
                 speedup_vs_sequential=max(orr) / max(seq))
        print(json.dumps(r), flush=True)
        res["use_case"].append(r)
        del own, ones
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
