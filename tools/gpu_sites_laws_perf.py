"""What a noise law per site costs (SiteTargets(per_site_law=True), include/bh_engine_sites_laws.h), and chain-iterations/s of many
stations whose installed laws differ.

  (a) the mechanism: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/gpu_sites_laws_perf.py
      --trace MODE`, a run per MODE, makes five evaluate calls of 4096 ten-layer models over 64 sites on a Rayleigh phase curve of
      30 periods beside a receiver function under the Gauss law (four correlation classes) of n = 60 samples (one wavefront per
      model: like_small_sites_*_kernel) or n = 200 (one workgroup per model: like_sites_*_kernel):
        classes_60 / classes_200      the existing class path (like_kernel_c.hip): the yardstick
        laws_60 / laws_200            the same laws at every site THROUGH the law table (like_kernel_l.hip): what the lookup costs
        mixed_60 / mixed_200          the laws mixed over the sites (nocorr / scaled / exp on the curve; Gauss / exp / nocorr /
                                      scaled on the receiver function)
      `--trace-stats MODE=CSV,... --out FILE` puts the rows of the likelihood kernels into FILE's "mechanism".
  (b) the use case: Rayleigh phase + Rayleigh group dispersion + P receiver function, S sites x 8 chains, the priors -- hence the
      installed laws -- of four kinds spread over the sites: error bars and corr 0 with the receiver function's correlation fixed at
      0.98 (scaled / Gauss); no error bars, corr 0, 0.92 (nocorr / Gauss); both correlations ranged (exp / exp); corr 0 and no
      receiver function (nocorr):
        own          the sites in ONE DeviceChains (missing=True, per_site_law=True, a dict of priors per site)
        sequential   the sites as one-site DeviceChains runs over the targets each has, made one after another
  (c) the table's own cost in a chain run: the SAME law at every site (nocorr / nocorr / Gauss 0.98), once with per_site_law=True
      and once without the flag, alternating.

    python tools/gpu_sites_laws_perf.py [--sites 8,64] [--iters 300] [--repeat 3] [--out profiles/sites_laws_perf.json]

Each run is repeated `--repeat` times, the two sides alternating; the best and every repeat are reported with the spread
(max - min) / max.  Only the iterations are timed.  No threshold is asserted: the figures are what was measured.
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
TRACE_MODES = ["classes_60", "laws_60", "mixed_60", "classes_200", "laws_200", "mixed_200"]
KERNELS = ("like_",)
# the four kinds of station of (b): (error bars on the curves, swdnoise_corr, rfnoise_corr or None: no receiver function)
KINDS = ((True, 0., 0.98), (False, 0., 0.92), (False, (0.1, 0.6), (0.35, 0.75)), (False, 0., None))


def own_periods(s):
    """15..30 periods between 1..4.5 s and 22..41 s"""
    k = 15 + (7 * s) % 16
    return np.linspace(1.0 + 0.5 * (s % 8), 22.0 + (5 * s) % 20, k)


def slots(g, s, kind):
    """[Rayleigh phase, Rayleigh group, P receiver function] of site s of kind `kind`"""
    yerr, _, rfcorr = kind
    rs = np.random.RandomState(1000 + s)
    xs, ys = np.asarray(g["xsw"], dtype=float), np.asarray(g["ysw"], dtype=float)
    xp, xg = own_periods(s), own_periods(s + 3)
    e1 = rs.uniform(0.01, 0.03, xp.size) if yerr else None
    e2 = rs.uniform(0.01, 0.03, xg.size) if yerr else None
    t1 = bh.RayleighDispersionPhase(xp, np.interp(xp, xs, ys) + rs.normal(0, 0.02, xp.size), yerr=e1)
    t2 = bh.RayleighDispersionGroup(xg, 0.9 * np.interp(xg, xs, ys) + rs.normal(0, 0.02, xg.size), yerr=e2)
    t3 = bh.PReceiverFunction(g["xrf"], g["yrf"] + rs.normal(0, 0.01, g["yrf"].size))
    t3.moddata.plugin.set_modelparams(gauss=1.0, p=6.4)
    return [t1, t2, None if rfcorr is None else t3]


def priors_of(kind):
    _, swdcorr, rfcorr = kind
    return dict(PRIORS, swdnoise_corr=swdcorr, rfnoise_corr=PRIORS["rfnoise_corr"] if rfcorr is None else rfcorr)


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
    S, B, K = 64, 4096, 30
    rs = np.random.RandomState(1)
    nlay, h, vp, vs, rho = synth_models(rs, B, 10, ragged=True)
    site = rs.randint(0, S, B).astype(np.int32)
    mats = []
    for c in CORR:
        v = Valuation()
        v.init_covariance_gauss(c, n, rcond=1e-5)
        mats.append((np.ascontiguousarray(v.corr_inv), float(v.logcorr_det)))
    d0 = dict(kind=E.TARGET_SWD, law=E.LAW_NOCORR, n=K, x=np.ones(K), yobs=np.zeros(K), iwave=2, igr=0)
    d1 = dict(kind=E.TARGET_RF, law=E.LAW_GAUSS, n=n, waveno=0, p=6.4, gauss=2.5, tshift=5.0, nsamp=512, fsamp=5.0, yobs=np.zeros(n),
              rinv=mats[0][0], logdet_r=mats[0][1])
    cnt = np.tile(np.array([K, n], np.int32), (S, 1))
    x, yobs = np.zeros((S, K + n)), rs.normal(0, 0.05, (S, K + n))
    x[:, :K] = np.linspace(2.0, 60.0, K)
    yobs[:, :K] += 3.0 + 0.02 * x[:, :K]
    yerr = rs.uniform(0.02, 0.06, (S, K + n))
    p = np.tile([0.0, 6.4], (S, 1))
    law = np.tile(np.array([E.LAW_NOCORR, E.LAW_GAUSS], np.int32), (S, 1))
    class_of = (np.arange(S) % 4).astype(np.int32)
    if kind == "mixed":
        law[:, 0] = np.array([E.LAW_NOCORR, E.LAW_NOCORR_SCALED, E.LAW_EXP])[np.arange(S) % 3]
        law[:, 1] = np.array([E.LAW_GAUSS, E.LAW_EXP, E.LAW_GAUSS, E.LAW_NOCORR, E.LAW_GAUSS, E.LAW_NOCORR_SCALED])[np.arange(S) % 6]
        class_of[law[:, 1] != E.LAW_GAUSS] = -1
    eng = E.default_engine(0)
    eng.set_targets([d0, d1])
    eng.set_sites_missing_gauss(cnt, x, yobs, yerr)
    eng.set_sites_rf(p, np.zeros((S, 2)))
    if kind != "classes":
        eng.set_sites_laws(law, yerr)
    eng.set_sites_gauss(1, class_of, np.stack([m[0] for m in mats]), np.array([m[1] for m in mats]))
    noise = np.tile([0.3, 0.05, 0.3, 0.05], (B, 1))
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
    res["mechanism"] = dict(shape="B = 4096 ragged ten-layer models over 64 sites, a Rayleigh phase curve of 30 periods beside a receiver "
                                  "function of n samples under the Gauss law (four classes), every call five times; duration per "
                                  "dispatch of the likelihood kernel.  classes_n: the existing class path; laws_n: the same laws through "
                                  "the law table; mixed_n: the laws mixed over the sites", modes=rows)
    for n in ("60", "200"):
        if all(k + "_" + n in rows for k in ("classes", "laws", "mixed")):
            avg = {k: sum(r["avg_us"] for r in rows[k + "_" + n]) for k in ("classes", "laws", "mixed")}
            mn = {k: sum(r["min_us"] for r in rows[k + "_" + n]) for k in ("classes", "laws", "mixed")}
            res["mechanism"]["n" + n] = dict(classes_us=avg["classes"], laws_us=avg["laws"], mixed_us=avg["mixed"],
                                             classes_min_us=mn["classes"], laws_min_us=mn["laws"], mixed_min_us=mn["mixed"],
                                             laws_over_classes=avg["laws"] / avg["classes"], mixed_over_classes=avg["mixed"] / avg["classes"])
    print(json.dumps({k: v for k, v in res["mechanism"].items() if k.startswith("n")}), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


def spread(v):
    return (max(v) - min(v)) / max(v)


def mixed_runs(g, S, a):
    """(b): S stations of the four kinds in one run against their one-site runs made one after another"""
    kinds = [KINDS[s % 4] for s in range(S)]
    priors = [priors_of(k) for k in kinds]
    st = bh.SiteTargets([slots(g, s, kinds[s]) for s in range(S)], per_site_x="all", per_site_rf=True, missing=True, per_site_law=True)
    own = DeviceChains(st, a.chains, INIT, priors, seed=5)
    ones = [DeviceChains(bh.JointTarget([t for t in slots(g, s, kinds[s]) if t is not None]), a.chains, INIT, priors[s], seed=5,
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
        print("[%d sites, mixed laws] repeat %d done" % (S, len(seq)), file=sys.stderr, flush=True)
    law = st.site_law_arrays()
    r = dict(sites=S, chains=S * a.chains, spec_depth=own.depth, one_site_spec_depth=ones[0].depth,
             laws_per_slot=[sorted(set(int(v) for v, p in zip(law[:, i], st.present[:, i]) if p)) for i in range(law.shape[1])],
             classes=int(st.gauss_class_arrays()[2][1].shape[0]), sites_without_rf=int((~st.present[:, 2]).sum()),
             own_rate=max(own_rates), sequential_rate=max(seq), own_rates=own_rates, sequential_rates=seq,
             own_spread=spread(own_rates), sequential_spread=spread(seq))
    r["speedup_vs_sequential"] = r["own_rate"] / r["sequential_rate"]
    return r


def uniform_runs(g, S, a):
    """(c): one law at every site, through the law table and without the flag"""
    kind = (False, 0., 0.98)
    priors = [priors_of(kind) for _ in range(S)]
    runs = {}
    for flag in (True, False):
        st = bh.SiteTargets([slots(g, s, kind) for s in range(S)], per_site_x="all", per_site_rf=True, missing=True, per_site_corr=True,
                            per_site_law=flag)
        runs[flag] = DeviceChains(st, a.chains, INIT, priors, seed=5)
    for dc in runs.values():
        timed(dc, a.warm)
    rates = {True: [], False: []}
    for _ in range(a.repeat):
        for flag in (True, False):
            timed(runs[flag], 5)    # (takes the engine's registration back: outside the timed part)
            n, dt = timed(runs[flag], a.iters)
            rates[flag].append(n / dt)
        print("[%d sites, one law] repeat %d done" % (S, len(rates[True])), file=sys.stderr, flush=True)
    r = dict(sites=S, chains=S * a.chains, spec_depth=runs[True].depth, table_rate=max(rates[True]), plain_rate=max(rates[False]),
             table_rates=rates[True], plain_rates=rates[False], table_spread=spread(rates[True]), plain_spread=spread(rates[False]))
    r["table_over_plain"] = r["table_rate"] / r["plain_rate"]
    return r


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
                "workload": "R phase + R group dispersion + P-RF (201 samples, rcond 1e-5), 1..20 layers, 15..30 periods per site and "
                            "curve.  mixed: stations of four kinds in turn -- error bars, corr 0, rf corr 0.98 (scaled / Gauss); corr 0, "
                            "0.92 (nocorr / Gauss); both correlations ranged (exp / exp); corr 0 and no receiver function.  uniform: "
                            "corr 0 without error bars and rf corr 0.98 at every site, with and without per_site_law",
                "mixed": [], "uniform": []})
    for S in [int(x) for x in a.sites.split(",")]:
        for key, fn in (("mixed", mixed_runs), ("uniform", uniform_runs)):
            r = fn(g, S, a)
            print(json.dumps(r), flush=True)
            res[key].append(r)
            if a.out:                   # (after every run: a run cut short keeps what was measured)
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
