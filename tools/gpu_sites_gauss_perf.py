"""What a Gauss-law noise correlation per site costs (SiteTargets(per_site_corr=True), include/bh_engine_sites_gauss.h), and
chain-iterations/s of many stations that fix their own correlation.

  (a) the mechanism: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/gpu_sites_gauss_perf.py
      --trace MODE`, a run per MODE, makes five evaluate calls of 4096 ten-layer models over 64 sites on one receiver function
      under the Gauss law, n = 1024 samples (the 128 x 128 form of the contraction) or n = 100 (the 64 x 64 form):
        sites_1024 / sites_100        the existing sites contraction (no class table): the yardstick
        one_1024 / one_100            every site in ONE class through the class path: what the mechanism costs
        four_1024 / four_100          four classes spread over the sites: the padded tiles on top
      `--trace-stats MODE=CSV,... --out FILE` puts the rows of the contraction, of the three grouping launches and of the
      likelihood kernel into FILE's "mechanism".
  (b) the use case: Rayleigh phase + Rayleigh group dispersion + P receiver function under the Gauss law, S sites x 8 chains, four
      correlation values (0.90 / 0.94 / 0.96 / 0.98) spread over the sites, every fourth site without a receiver function:
        own          the sites in ONE DeviceChains (missing=True, per_site_corr=True, a dict of priors per site)
        sequential   the sites as one-site DeviceChains runs over the targets each has, made one after another

    python tools/gpu_sites_gauss_perf.py [--sites 8,64] [--iters 300] [--repeat 3] [--out profiles/sites_gauss_perf.json]

Each run is repeated `--repeat` times, own and sequential alternating; the best and every repeat are reported.  Only the
iterations are timed.
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
from bayhunter_amd.Targets import Valuation  # noqa: E402

PRIORS = dict(vpvs=(1.4, 2.1), layers=(1, 20), vs=(2, 5), z=(0, 60), rfnoise_corr=0.98,
              rfnoise_sigma=(1e-5, 0.05), swdnoise_corr=0., swdnoise_sigma=(1e-5, 0.1))
INIT = dict(nchains=1, iter_burnin=5000, iter_main=100, acceptance=(40, 80), thickmin=0.1, lvz=0.1, hvz=None, rcond=1e-5,
            maxmodels=10)
CORR = (0.90, 0.94, 0.96, 0.98)
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "chain_golden.npz")
TRACE_MODES = ["sites_1024", "one_1024", "four_1024", "sites_100", "one_100", "four_100"]
KERNELS = ("gauss_quad", "gauss_class", "like_")


def own_periods(s):
    """15..30 periods between 1..4.5 s and 22..41 s"""
    k = 15 + (7 * s) % 16
    return np.linspace(1.0 + 0.5 * (s % 8), 22.0 + (5 * s) % 20, k)


def corr_of(s):
    return CORR[(s // 4 + s) % 4]


def lacks_rf(s):
    return s % 4 == 3


def slots(g, s):
    """[Rayleigh phase, Rayleigh group, P receiver function] of site s, None where it has no receiver function"""
    rs = np.random.RandomState(1000 + s)
    xs, ys = np.asarray(g["xsw"], dtype=float), np.asarray(g["ysw"], dtype=float)
    xp, xg = own_periods(s), own_periods(s + 3)
    t1 = bh.RayleighDispersionPhase(xp, np.interp(xp, xs, ys) + rs.normal(0, 0.02, xp.size))
    t2 = bh.RayleighDispersionGroup(xg, 0.9 * np.interp(xg, xs, ys) + rs.normal(0, 0.02, xg.size))
    t3 = bh.PReceiverFunction(g["xrf"], g["yrf"] + rs.normal(0, 0.01, g["yrf"].size))
    t3.moddata.plugin.set_modelparams(gauss=1.0, p=6.4)
    return [t1, t2, None if lacks_rf(s) else t3]


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
    from bayhunter_amd.synth import synth_models
    kind, n = mode.split("_")
    n = int(n)
    S, B = 64, 4096
    rs = np.random.RandomState(1)
    nlay, h, vp, vs, rho = synth_models(rs, B, 10, ragged=True)
    site = rs.randint(0, S, B).astype(np.int32)
    mats = []
    for c in CORR:
        v = Valuation()
        v.init_covariance_gauss(c, n, rcond=1e-5)
        mats.append((np.ascontiguousarray(v.corr_inv), float(v.logcorr_det)))
    desc = dict(kind=E.TARGET_RF, law=E.LAW_GAUSS, n=n, waveno=0, p=6.4, gauss=2.5, tshift=5.0, nsamp=2048 if n > 512 else 512,
                fsamp=20.0 if n > 512 else 5.0, yobs=rs.normal(0, 0.05, n), rinv=mats[0][0], logdet_r=mats[0][1])
    eng = E.default_engine(0)
    eng.set_targets([desc])
    eng.set_sites(rs.normal(0, 0.05, (S, n)))
    if kind == "one":
        eng.set_sites_gauss(0, np.zeros(S, np.int32), mats[0][0][None], np.array([mats[0][1]]))
    elif kind == "four":
        eng.set_sites_gauss(0, (np.arange(S) % 4).astype(np.int32), np.stack([m[0] for m in mats]), np.array([m[1] for m in mats]))
    noise = np.tile([0.0, 0.05], (B, 1))
    for _ in range(5):
        eng.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho)
    eng.synchronize()
    print(json.dumps(dict(mode=mode, models=B, sites=S, n=n)), flush=True)


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
    res["mechanism"] = dict(shape="B = 4096 ragged ten-layer models over 64 sites, one receiver function of n samples under the Gauss "
                                  "law, every call five times; duration per dispatch.  sites_n: the existing sites contraction; "
                                  "one_n: every site in one class through the class path; four_n: four classes", modes=rows)

    def per_call(mode, key):
        return sum(r["avg_us"] for r in rows.get(mode, []) if key in r["kernel"])
    for n in ("1024", "100"):
        if all(k + "_" + n in rows for k in ("sites", "one", "four")):
            base = per_call("sites_" + n, "gauss_quad")
            res["mechanism"]["n" + n] = dict(
                sites_contraction_us=base, one_contraction_us=per_call("one_" + n, "gauss_quad"), one_grouping_us=per_call("one_" + n, "gauss_class"),
                four_contraction_us=per_call("four_" + n, "gauss_quad"), four_grouping_us=per_call("four_" + n, "gauss_class"),
                one_over_sites=(per_call("one_" + n, "gauss_quad") + per_call("one_" + n, "gauss_class")) / base,
                four_over_sites=(per_call("four_" + n, "gauss_quad") + per_call("four_" + n, "gauss_class")) / base)
    print(json.dumps({k: v for k, v in res["mechanism"].items() if k.startswith("n")}), flush=True)
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
    g = np.load(GOLDEN)
    res = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res.update({"chains_per_site": a.chains, "iters": a.iters, "repeat": a.repeat,
                "workload": "R phase + R group dispersion + P-RF under the Gauss law (201 samples, rcond 1e-5), 1..20 layers, 15..30 "
                            "periods per site and curve; the noise correlation fixed at 0.90 / 0.94 / 0.96 / 0.98 over the sites, every "
                            "fourth site without the receiver function", "runs": []})
    for S in [int(x) for x in a.sites.split(",")]:
        priors = [dict(PRIORS, rfnoise_corr=corr_of(s)) for s in range(S)]
        st = bh.SiteTargets([slots(g, s) for s in range(S)], per_site_x="all", per_site_rf=True, missing=True, per_site_corr=True)
        own = DeviceChains(st, a.chains, INIT, priors, seed=5)
        ones = [DeviceChains(bh.JointTarget([t for t in slots(g, s) if t is not None]), a.chains, INIT, priors[s], seed=5,
                             chain_offset=s * a.chains) for s in range(S)]
        timed(own, a.warm)
        for one in ones:
            one.targets._register()     # (a one-site run registers its targets when it is made: the engine has changed hands since)
            timed(one, a.warm)
        own_rates, seq = [], []
        for _ in range(a.repeat):       # alternating: drifts of the clock or the host hit both alike
            timed(own, 5)               # (the many-site run takes the engine's registration back: outside the timed part)
            n, dt = timed(own, a.iters)
            own_rates.append(n / dt)
            seq_n, seq_dt = 0, 0.0
            for one in ones:
                one.targets._register()
                timed(one, 5)
                n1, dt1 = timed(one, a.iters)
                seq_n += n1
                seq_dt += dt1
            seq.append(seq_n / seq_dt)
            print("[%d sites] repeat %d done" % (S, len(seq)), file=sys.stderr, flush=True)
        spread = lambda v: (max(v) - min(v)) / max(v)
        classes = st.gauss_class_arrays()[2]
        r = dict(sites=S, chains=S * a.chains, spec_depth=own.depth, one_site_spec_depth=ones[0].depth,
                 classes=int(classes[1].shape[0]), sites_without_rf=int(sum(lacks_rf(s) for s in range(S))),
                 own_rate=max(own_rates), sequential_rate=max(seq), own_rates=own_rates, sequential_rates=seq,
                 own_spread=spread(own_rates), sequential_spread=spread(seq))
        r["speedup_vs_sequential"] = r["own_rate"] / r["sequential_rate"]
        print(json.dumps(r), flush=True)
        res["runs"].append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
