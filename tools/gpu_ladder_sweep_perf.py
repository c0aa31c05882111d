"""The exchange sweeps of tempered chains: what the one-kernel sweep (DeviceChains(ladder_adapt=)) costs beside the torch sweep
(parallel.DeviceExchange), and what the adaptation of the ladders buys.  Workload: bench.py's c5_full targets, 64 ladders x 8
temperatures = 512 chains on one GPU, bare iterate().

  cost    swap_every in {1, 5, 20}: (B) ladder_adapt=None, the torch sweep; (A) ladder_adapt={"every": 0}, the kernel, counting only.
          One DeviceChains each, burn-in untimed, then --reps segments of --iters main-phase iterations, A and B alternating
          segment by segment; chain-iterations/s, best of the segments with their spread.  The bar: A no slower than B by more
          than the spread of B's segments, at every swap_every.  The final states of A and B are compared bit for bit.
  adapt   ladders started linear in beta (1 .. 1/30): ladder_adapt={"every": 0} beside the defaults, equal iteration counts,
          record="device": ladder_diagnostics()' round_trips and the ladder_swaps() rates of the main phase.  Reported, no bar.
  --trace N        N sweeps of each route on synthetic likes, nothing else: run it under `rocprofv3 --kernel-trace --stats`
  --summarize DIR  condense that run's *kernel_stats.csv into --out (profiles/ladder_sweep_kernels.txt)

    python tools/gpu_ladder_sweep_perf.py [--sections cost adapt] [--out profiles/ladder_sweep_perf.json]
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LADDERS, RUNGS = 64, 8


def chains(eng, betas, burnin, main, swap_every, ladder_adapt, record="host", maxmodels=None):
    """DeviceChains on bench.py's chain targets (c5_full): Rayleigh and Love phase velocities and a receiver function"""
    import bayhunter_amd as bh
    from bayhunter_amd.device_chains import DeviceChains
    from bayhunter_amd.synth import RF_TIME, SEED, SWD_PERIODS, true_model
    nlay, h, vp, vs, rho = true_model(10)
    nrs = np.random.RandomState(SEED + 2)
    ys = {}
    for name, iwave in (("r", 2), ("l", 1)):
        y, _ = eng.swd_batch(nlay, h, vp, vs, rho, SWD_PERIODS, iwave, 0)
        ys[name] = y[0] + nrs.normal(0, 0.012, SWD_PERIODS.size)
    yrf = eng.rf_batch(nlay, h, vp, vs, rho, 6.4, 2.5, 2048, 20.0, 5.0, 0, RF_TIME.size)[0] + nrs.normal(0, 0.005, RF_TIME.size)
    t3 = bh.PReceiverFunction(RF_TIME, yrf)
    t3.moddata.plugin.set_modelparams(gauss=2.5, p=6.4)
    jt = bh.JointTarget([bh.RayleighDispersionPhase(SWD_PERIODS, ys["r"]), bh.LoveDispersionPhase(SWD_PERIODS, ys["l"]), t3], engine=eng)
    priors = dict(vpvs=(1.4, 2.1), layers=(1, 20), vs=(2, 5), z=(0, 60), rfnoise_corr=(0.35, 0.75), rfnoise_sigma=(1e-5, 0.05),
                  swdnoise_corr=0., swdnoise_sigma=(1e-5, 0.1))
    init = dict(iter_burnin=burnin, iter_main=main, acceptance=(40, 45), thickmin=0.1, lvz=None, hvz=None, rcond=None,
                maxmodels=maxmodels or max(1, main // 100))
    return DeviceChains(jt, LADDERS * RUNGS, init, priors, seed=20260927, betas=np.tile(betas, LADDERS),
                        ladder=np.repeat(np.arange(LADDERS), RUNGS), swap_every=swap_every, ladder_adapt=ladder_adapt, record=record)


def section_cost(eng, torch, a):
    geometric = 1.0 / np.geomspace(1.0, 30.0, RUNGS)

    def fence():
        eng.synchronize()
        torch.cuda.synchronize()

    out = []
    for swap_every in (1, 5, 20):
        runs = {"B": chains(eng, geometric, a.warmup, a.iters * a.reps, swap_every, None),
                "A": chains(eng, geometric, a.warmup, a.iters * a.reps, swap_every, {"every": 0})}
        for dc in runs.values():
            while dc.iiter < 0:
                dc.iterate()
        fence()
        times = {"A": [], "B": []}
        for rep in range(a.reps):
            for name in (("B", "A") if rep % 2 == 0 else ("A", "B")):
                dc = runs[name]
                stop = min(dc.iter_phase2, (dc.iiter // a.iters + 1) * a.iters)
                fence()
                i0, t0 = dc.iiter, time.perf_counter()
                while dc.iiter < stop:
                    dc.iterate()
                fence()
                times[name].append((time.perf_counter() - t0) / (dc.iiter - i0))
        sa, sb = runs["A"].state_host(), runs["B"].state_host()
        same = all((sa[k] is None and sb[k] is None) or np.array_equal(sa[k], sb[k], equal_nan=True) for k in sa)
        C = LADDERS * RUNGS
        rate = {k: dict(best=C / min(v), all=[C / t for t in v], spread=C / min(v) - C / max(v)) for k, v in times.items()}
        out.append(dict(swap_every=swap_every, sweeps_per_route=runs["A"].sweep, chain_iterations_per_s=rate,
                        seconds_per_iteration={k: dict(best=min(v), all=v, spread=max(v) - min(v)) for k, v in times.items()},
                        a_over_b_time=min(times["A"]) / min(times["B"]),
                        bar_met=bool(min(times["A"]) <= min(times["B"]) + (max(times["B"]) - min(times["B"]))),
                        same_final_state=bool(same), nswaps=dict(A=int(runs["A"].nswaps), B=int(runs["B"].nswaps))))
        print(json.dumps(out[-1]), flush=True)
        del runs
    return dict(workload="%d ladders x %d temperatures (geometric 1 .. 1/30), bench.py's c5_full targets, bare iterate()" % (LADDERS, RUNGS),
                iterations_per_segment=a.iters, segments=a.reps, burnin_untimed=a.warmup,
                routes=dict(A="ladder_adapt={'every': 0}: one kernel per sweep, counting only", B="ladder_adapt=None: parallel.DeviceExchange"),
                bar="A no slower than B by more than the spread of B's segments, at every swap_every",
                bar_met=bool(all(r["bar_met"] for r in out)), results=out)


def section_adapt(eng, a):
    linear = np.linspace(1.0, 1.0 / 30.0, RUNGS)
    out = {}
    for name, opt in (("linear", {"every": 0}), ("adapted", {})):
        dc = chains(eng, linear, a.adapt_burnin, a.adapt_main, a.adapt_swap_every, opt, record="device", maxmodels=a.adapt_main // 2)
        dc.run()
        sw, diag = dc.ladder_swaps(), dc.ladder_diagnostics()
        rate = np.array(sw["rate"])[:, 1, :]                                   # [ladder][pair], main phase
        out[name] = dict(ladder_adapt=opt, betas_of_ladder_0=[float(b) for b in sw["betas"][0]],
                         round_trips_total=int(diag["ladders"]["round_trips"].sum()),
                         ladders_without_a_round_trip=int(sum(diag["ladders"]["round_trips"][8 * k:8 * k + 8].sum() == 0 for k in range(LADDERS))),
                         rate_per_pair_mean_over_ladders=[float(x) for x in np.nanmean(rate, axis=0)],
                         smallest_pair_rate=float(np.nanmin(rate)), largest_pair_rate=float(np.nanmax(rate)),
                         mean_spread_within_a_ladder=float(np.mean(np.nanmax(rate, axis=1) - np.nanmin(rate, axis=1))),
                         adaptations=int(sw["adaptations"].sum()), skipped=int(sw["skipped"].sum()), nswaps=int(dc.nswaps),
                         recorded_rows=int(dc.samples("p2")["likes"].shape[0]))
        print(json.dumps({name: out[name]}), flush=True)
        del dc
    return dict(workload="%d ladders x %d temperatures started linear in beta (1 .. 1/30), bench.py's c5_full targets" % (LADDERS, RUNGS),
                iter_burnin=a.adapt_burnin, iter_main=a.adapt_main, swap_every=a.adapt_swap_every, bar=None, results=out)


def trace(eng, torch, n):
    """n sweeps of each route on 512 chains with synthetic likes: every torch kernel of this process is a kernel of route B"""
    from bayhunter_amd import parallel as P
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(1)
    ladder = np.repeat(np.arange(LADDERS), RUNGS)
    beta0 = np.tile(1.0 / np.geomspace(1.0, 30.0, RUNGS), LADDERS)
    likes = torch.from_numpy(-rs.gamma(5.0, size=(n, beta0.size)) * 10.0).to(dev)
    b_t, b_k = torch.from_numpy(beta0).to(dev), torch.from_numpy(beta0.copy()).to(dev)
    ex_t = P.DeviceExchange(ladder, 3, slice(0, beta0.size), dev)
    ex_k = P.KernelExchange(eng, ladder, 3, dev)
    for s in range(n):
        ex_t.sweep(likes[s], b_t, s)
    torch.cuda.synchronize()
    for s in range(n):
        ex_k.sweep(likes[s], b_k, s)
    torch.cuda.synchronize()
    assert torch.equal(b_t, b_k) and int(ex_t.nacc.item()) == int(ex_k.nacc.item())
    print(json.dumps(dict(sweeps=n, nacc=int(ex_k.nacc.item()))))


def summarize(d, n, out):
    """the kernel statistics of a --trace run: the sweep kernel beside the summed torch kernels of a DeviceExchange sweep"""
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        raise SystemExit("no *kernel_stats.csv below %s" % d)
    rows = list(csv.DictReader(open(files[0])))
    mine = [r for r in rows if "ladder_sweep_kernel" in r["Name"]]
    other = [r for r in rows if "ladder_sweep_kernel" not in r["Name"]]
    rt = [r for r in other if r["Name"].startswith("__amd_rocclr")]      # the runtime's copy and fill kernels
    th = [r for r in other if not r["Name"].startswith("__amd_rocclr")]
    per = lambda rs: (sum(int(r["Calls"]) for r in rs) / float(n), sum(int(r["TotalDurationNs"]) for r in rs) / 1e3 / n)
    lines = ["# one `rocprofv3 --kernel-trace --stats` run of `tools/gpu_ladder_sweep_perf.py --trace %d`: %d sweeps of each route on %d"
             % (n, n, LADDERS * RUNGS),
             "# chains (%d ladders x %d temperatures) with synthetic likes.  The at::native kernels all belong to the" % (LADDERS, RUNGS),
             "# parallel.DeviceExchange sweeps; the runtime's own copy kernels (__amd_rocclr_*) are the copies of those sweeps (clone, copy_,",
             "# the upload of the log-uniforms) and, for a small part, the set-up and the chunked uploads of both routes: listed apart.",
             "ladder_sweep_kernel: %d calls, %.2f us each" % (int(mine[0]["Calls"]), float(mine[0]["AverageNs"]) / 1e3) if mine
             else "ladder_sweep_kernel: not in the trace",
             "torch kernels of a DeviceExchange sweep: %.1f launches, %.2f us summed per sweep" % per(th),
             "runtime copy kernels, both routes, per sweep of one route: %.1f launches, %.2f us" % per(rt)]
    for r in sorted(other, key=lambda r: -int(r["TotalDurationNs"])):
        lines.append("  %6d calls %9.2f us each  %s" % (int(r["Calls"]), float(r["AverageNs"]) / 1e3, r["Name"][:150]))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:7]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", nargs="*", default=["cost", "adapt"], choices=["cost", "adapt"])
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--adapt-burnin", type=int, default=4000)
    ap.add_argument("--adapt-main", type=int, default=2000)
    ap.add_argument("--adapt-swap-every", type=int, default=2)
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--summarize", default=None)
    ap.add_argument("--sweeps", type=int, default=200, help="--summarize: the N of the traced run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize, a.sweeps, a.out or "ladder_sweep_kernels.txt")
    import torch
    from bayhunter_amd import engine as E
    eng = E.default_engine(0)
    if a.trace:
        return trace(eng, torch, a.trace)
    res = {}
    if "cost" in a.sections:
        res["sweep_cost"] = section_cost(eng, torch, a)
    if "adapt" in a.sections:
        res["adaptation"] = section_adapt(eng, a)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
