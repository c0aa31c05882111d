"""Chain-iterations/s of many stations at once when every station's Rayleigh ellipticity (H/V) has its own periods or is absent
(SiteTargets(per_site_ellip=True), include/bh_engine_sites_ellip.h), and the fused call through the table against the existing
shared-period path.  Workload: Rayleigh phase velocities + ellipticity, prior-like transdimensional models (1..20 layers), the
stations' curves of 15..30 periods from different bands, S sites x 8 chains, bare iterate().  Three variants per S, each against
its stations' one-site DeviceChains runs made one after another:

  (A) own_shared   every station's ellipticity at its own phase periods: the ellipticity reads the phase slot's search
  (B) own_private  the ellipticity at other periods than the phase slot's: a search of its own
  (C) own_missing  as A, every fourth station without the ellipticity

    python tools/gpu_sites_ellip_perf.py [--sites 8,64] [--iters 200] [--repeat 3] [--out profiles/sites_ellip_perf.json]

Each run is repeated `--repeat` times, the variants alternating; the best and every repeat are reported with the spread.  Only the
iterations are timed.

  --fused  one fused call of 4096 ten-layer models over 64 stations that all share one period set (21 periods on both slots),
through the flag (the table; the search shared by bh_plan_ellip_sites) and through the existing shared-period path
(SiteTargets without per_site_x), `--repeat` x 20 calls each, alternating.  THE BAR: through the table no slower than the existing
path by more than the spread of the EXISTING path's repeats.
  `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/gpu_sites_ellip_perf.py --fused-only MODE`
(MODE = table or existing, every call five times) gives the ellipticity kernel's time.
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

PRIORS = dict(vpvs=(1.4, 2.1), layers=(1, 20), vs=(2, 5), z=(0, 60), swdnoise_corr=0., swdnoise_sigma=(1e-5, 0.1),
              ellnoise_corr=0., ellnoise_sigma=(1e-3, 0.2))
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "chain_golden.npz")
VARIANTS = ("own_shared", "own_private", "own_missing")


def own_periods(s):
    """15..30 periods between 1..4.5 s and 22..41 s"""
    k = 15 + (7 * s) % 16
    return np.linspace(1.0 + 0.5 * (s % 8), 22.0 + (5 * s) % 20, k)


def row(g, s, variant):
    """station s: [Rayleigh phase, ellipticity or None]"""
    rs = np.random.RandomState(1000 + s)
    xs, ys = np.asarray(g["xsw"], dtype=float), np.asarray(g["ysw"], dtype=float)
    xp = own_periods(s)
    xe = own_periods(s + 3) if variant == "own_private" else xp
    t1 = bh.RayleighDispersionPhase(xp, np.interp(xp, xs, ys) + rs.normal(0, 0.02, xp.size))
    if variant == "own_missing" and s % 4 == 3:
        return [t1, None]
    return [t1, bh.RayleighEllipticity(xe, 0.7 + 0.004 * xe + rs.normal(0, 0.01, xe.size), fused=True)]


def timed(dc, iters):
    dc.engine.synchronize()
    t0 = time.perf_counter()
    start = dc.iiter
    while dc.iiter - start < iters:
        dc.iterate()
    dc.engine.synchronize()
    return dc.C * (dc.iiter - start), time.perf_counter() - t0


def spread(v):
    return (max(v) - min(v)) / max(v)


def fused_sets():
    from bayhunter_amd.synth import SWD_PERIODS
    per = np.asarray(SWD_PERIODS, dtype=float)[:21]
    out = {}
    for mode in ("existing", "table"):
        sites = []
        for s in range(64):
            ts = [bh.RayleighDispersionPhase(per, 3.0 + 0.01 * per + 0.001 * s), bh.RayleighEllipticity(per, 0.7 + 0.004 * per, fused=True)]
            for t in ts:
                t.set_noise_law("nocorr")
            sites.append(ts)
        out[mode] = bh.SiteTargets(sites) if mode == "existing" else bh.SiteTargets(sites, per_site_x="all", per_site_ellip=True)
    return out


def fused_batch():
    from bayhunter_amd.synth import synth_models
    rs = np.random.RandomState(1)
    mods = synth_models(rs, 4096, 10, ragged=True)
    return mods, rs.randint(0, 64, 4096).astype(np.int32), np.tile([0.0, 0.05, 0.0, 0.07], (4096, 1))


def fused_only(mode):
    (nlay, h, vp, vs, rho), site_b, noise = fused_batch()
    st = fused_sets()[mode]
    for _ in range(5):
        st.evaluate_batch(nlay, h, vp, vs, noise, site_b, rho=rho)
    print(json.dumps(dict(mode=mode, launches=[(l["family"], l["role"], l["interleaved"]) for l in st.engine.last_swd_launches()])), flush=True)
    bh.default_engine(0).synchronize()


def fused(repeat, calls=20):
    (nlay, h, vp, vs, rho), site_b, noise = fused_batch()
    sets = fused_sets()
    ms = {k: [] for k in sets}
    for st in sets.values():
        st.evaluate_batch(nlay, h, vp, vs, noise, site_b, rho=rho)
    for _ in range(repeat):
        for k, st in sets.items():
            st.evaluate_batch(nlay, h, vp, vs, noise, site_b, rho=rho)   # (the registration changes hands: outside the timed part)
            t0 = time.perf_counter()
            for _ in range(calls):
                st.evaluate_batch(nlay, h, vp, vs, noise, site_b, rho=rho)
            ms[k].append((time.perf_counter() - t0) / calls * 1e3)
    r = dict(shape="one host call of 4096 ragged ten-layer models over 64 stations, Rayleigh phase + ellipticity at 21 shared periods; "
                   "ms per call, %d calls per repeat" % calls,
             existing_ms=min(ms["existing"]), table_ms=min(ms["table"]), existing_all=ms["existing"], table_all=ms["table"],
             existing_spread=spread(ms["existing"]), table_spread=spread(ms["table"]))
    r["table_cost"] = r["table_ms"] / r["existing_ms"] - 1.0
    r["bar_met"] = bool(r["table_ms"] <= max(ms["existing"]))    # no slower than the existing path's best by more than ITS spread
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", default="8,64")
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warm", type=int, default=30)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--fused", action="store_true")
    ap.add_argument("--fused-only", choices=["table", "existing"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.fused_only:
        fused_only(a.fused_only)
        return
    res = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    if a.fused:
        res["fused_call"] = fused(a.repeat)
        print(json.dumps(res["fused_call"]), flush=True)
    else:
        g = np.load(GOLDEN)
        init = dict(nchains=1, iter_burnin=5000, iter_main=100, acceptance=(40, 80), thickmin=0.1, lvz=0.1, hvz=None, rcond=None, maxmodels=10)
        res.update({"chains_per_site": a.chains, "iters": a.iters, "repeat": a.repeat,
                    "workload": "R phase + R ellipticity, 1..20 layers, 15..30 periods per station from different bands; bare iterate()",
                    "runs": []})
        for S in [int(x) for x in a.sites.split(",")]:
            runs = {v: DeviceChains(bh.SiteTargets([row(g, s, v) for s in range(S)], per_site_x="all", missing=True, per_site_ellip=True),
                                    a.chains, init, PRIORS, seed=5) for v in VARIANTS}
            rates = {v: [] for v in VARIANTS}
            for dc in runs.values():
                timed(dc, a.warm)
            for _ in range(a.repeat):       # alternating: drifts of the clock or the host hit all alike
                for v, dc in runs.items():
                    timed(dc, 5)            # (the engine's registration changes hands: outside the timed part)
                    n, dt = timed(dc, a.iters)
                    rates[v].append(n / dt)
            print("[%d sites] runs in one DeviceChains done" % S, file=sys.stderr, flush=True)
            r = dict(sites=S, chains=S * a.chains, spec_depth=runs["own_shared"].depth,
                     periods_per_site=[int(own_periods(s).size) for s in range(S)])
            for v in VARIANTS:
                ones = []
                for s in range(S):
                    one = DeviceChains([t for t in row(g, s, v) if t is not None], a.chains, init, PRIORS, seed=5, chain_offset=s * a.chains)
                    timed(one, a.warm)
                    ones.append(one)
                seq = []
                for _ in range(a.repeat):
                    seq_n, seq_dt = 0, 0.0
                    for one in ones:
                        timed(one, 5)
                        n1, dt1 = timed(one, a.iters)
                        seq_n += n1
                        seq_dt += dt1
                    seq.append(seq_n / seq_dt)
                del ones
                print("[%d sites] %s: one-site runs done" % (S, v), file=sys.stderr, flush=True)
                r[v] = dict(rate=max(rates[v]), rates=rates[v], spread=spread(rates[v]), sequential_rate=max(seq), sequential_rates=seq,
                            sequential_spread=spread(seq), speedup_vs_sequential=max(rates[v]) / max(seq))
            print(json.dumps(r), flush=True)
            res["runs"].append(r)
            if a.out:                       # (after every S: a long run that is cut short keeps what it measured)
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
