"""run() in chain-iterations/s with the thinned samples taken on the host (record="host": a synchronisation and eight copies per
snapshot, windows end at snapshot iterations) and on the device (record="device": include/bh_engine_chain_record.h), beside the
bare iterate() loop of the same session -- what bench.py times, which keeps no samples -- as the ceiling.

Workloads: bench.py's c4 and c5 set-ups on one GPU (Rayleigh + Love phase dispersion + P receiver function, up to 20 layers;
c4: 8 chains; c5: 64 chains, one rung of a tempering ladder each, exchange sweep every 100 iterations).
Thinning 1 (maxmodels >= iter_main: the reference's defaults and its tutorial keep every iteration) and 100 (bench.py's maxmodels).

    python tools/gpu_chain_record_perf.py [--burnin 1000] [--main 2000] [--repeat 3] [--out profiles/chain_record_perf.json]

Every (workload, thinning) step is a child process of its own under `timeout`; the first step that fails ends the measurement.
Inside a step host, device and iterate alternate `--repeat` times, each on a fresh DeviceChains with the same seed (the runs walk the
same trajectories); the best of each and the spread of its repeats, (max - min) / max, are reported.  run() is timed from its call
to the end of its closing synchronisation; `*_with_samples` adds samples("p1") and samples("p2"), the one copy of the store.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRIORS = dict(vpvs=(1.4, 2.1), layers=(1, 20), vs=(2, 5), z=(0, 60), rfnoise_corr=(0.35, 0.75), rfnoise_sigma=(1e-5, 0.05),
              swdnoise_corr=0., swdnoise_sigma=(1e-5, 0.1))
STEPS = [(w, t) for w in ("c4", "c5") for t in (1, 100)]


def bench_targets(eng, layers=10):
    """the observed data of bench.py's chain workloads"""
    import bayhunter_amd as bh
    from bayhunter_amd.synth import true_model, SWD_PERIODS, RF_TIME, SEED
    nlay, h, vp, vs, rho = true_model(layers)
    nrs = np.random.RandomState(SEED + 2)
    ys = {}
    for name, iwave in (("r", 2), ("l", 1)):
        y, _ = eng.swd_batch(nlay, h, vp, vs, rho, SWD_PERIODS, iwave, 0)
        ys[name] = y[0] + nrs.normal(0, 0.012, SWD_PERIODS.size)
    yrf = eng.rf_batch(nlay, h, vp, vs, rho, 6.4, 2.5, 2048, 20.0, 5.0, 0, RF_TIME.size)[0] + nrs.normal(0, 0.005, RF_TIME.size)
    t3 = bh.PReceiverFunction(RF_TIME, yrf)
    t3.moddata.plugin.set_modelparams(gauss=2.5, p=6.4)
    return bh.JointTarget([bh.RayleighDispersionPhase(SWD_PERIODS, ys["r"]), bh.LoveDispersionPhase(SWD_PERIODS, ys["l"]), t3], engine=eng)


def step(workload, thinning, burnin, main, repeat):
    from bayhunter_amd import engine as E
    from bayhunter_amd.device_chains import DeviceChains, record_rows
    eng = E.default_engine(0)
    jt = bench_targets(eng)
    C = 8 if workload == "c4" else 64
    kw = {}
    if workload == "c5":
        kw = dict(betas=np.full(C, 1.0), ladder=np.arange(C), swap_every=100)

    def make(record, b=burnin, m=main):
        init = dict(iter_burnin=b, iter_main=m, acceptance=(40, 45), thickmin=0.1, lvz=None, hvz=None, rcond=None,
                    maxmodels=m if thinning == 1 else max(1, m // thinning))
        dc = DeviceChains(jt, C, init, PRIORS, seed=20260927, record=record, **kw)
        assert m != main or dc.thinning == thinning, (dc.thinning, thinning)     # (the short warm-up runs thin as they may)
        return dc

    def run(record):
        dc = make(record)
        eng.synchronize()
        t0 = time.perf_counter()
        dc.run()
        t1 = time.perf_counter()
        rows = sum(dc.samples(p)["models"].shape[0] for p in ("p1", "p2"))
        t2 = time.perf_counter()
        assert rows == sum(record_rows(burnin, main, thinning))
        return C * (burnin + main) / (t1 - t0), C * (burnin + main) / (t2 - t0), dc.launches

    def bare():
        dc = make("host")
        eng.synchronize()
        t0 = time.perf_counter()
        while dc.iiter < dc.iter_phase2:
            dc.iterate()
        eng.synchronize()
        return C * (burnin + main) / (time.perf_counter() - t0), dc.launches

    for record in ("host", "device"):          # code objects, allocator, the engine's registration: outside the timed runs
        make(record, 60, 60).run().samples("p2")
    rates = {"host": [], "device": [], "host_with_samples": [], "device_with_samples": [], "iterate": []}
    launches = {}
    for _ in range(repeat):                    # alternating: drifts of the clock or the host hit all alike
        for record in ("host", "device"):
            r, rs, launches[record] = run(record)
            rates[record].append(r)
            rates[record + "_with_samples"].append(rs)
        r, launches["iterate"] = bare()
        rates["iterate"].append(r)
    out = dict(workload=workload, chains=C, thinning=thinning, iter_burnin=burnin, iter_main=main, repeat=repeat,
               spec_depth=make("host", 60, 60).depth, launches=launches, unit="chain-iterations/s")
    for k, v in rates.items():
        out[k] = max(v)
        out[k + "_repeats"] = v
        out[k + "_spread"] = (max(v) - min(v)) / max(v)
    out["device_over_host"] = out["device"] / out["host"]
    out["device_of_iterate_ceiling"] = out["device"] / out["iterate"]
    out["host_of_iterate_ceiling"] = out["host"] / out["iterate"]
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--burnin", type=int, default=1000)
    ap.add_argument("--main", type=int, default=2000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds a (workload, thinning) step may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="(internal) workload:thinning -- run that step in this process")
    a = ap.parse_args()
    if a.step:
        w, t = a.step.split(":")
        step(w, int(t), a.burnin, a.main, a.repeat)
        return 0
    res = {"what": "run() with record='host' / 'device' and the bare iterate() loop, chain-iterations/s over burn-in + main; "
                   "best of `repeat` fresh runs each, spread = (max - min) / max of the repeats",
           "iter_burnin": a.burnin, "iter_main": a.main, "repeat": a.repeat, "runs": []}
    for w, t in STEPS:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", "%s:%d" % (w, t),
               "--burnin", str(a.burnin), "--main", str(a.main), "--repeat", str(a.repeat)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            print("step %s thinning %d ended with status %d: nothing more is started" % (w, t, p.returncode), file=sys.stderr, flush=True)
            return p.returncode or 1
        r = json.loads(lines[-1][len("RESULT "):])
        print(json.dumps(r), flush=True)
        res["runs"].append(r)
        if a.out:                                # (after every step: a later step's failure keeps what was measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
