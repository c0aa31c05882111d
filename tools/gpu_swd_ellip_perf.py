"""What the Rayleigh ellipticity costs beside the search it follows (include/bh_engine_swd_ellip.h).  Workload: c2's shape --
4096 models of 10 layers from bench.py's generator, 30 periods -- on device arrays (torch), the engine's own stream.

  (S) the Rayleigh phase-velocity search, bh_swd_batch, with the engine's default search and arithmetic;
  (E) bh_swd_ellip(have_vel = 1, nsteps = 2) on the velocities (S) left: at most five evaluations of the compound vector per
      (model, period) against the search's ~50 rounds;
  (E0) the same with nsteps = 0: one evaluation.

Each is timed as --calls back-to-back calls between two synchronisations, --reps times, S and E alternating; best of the
repetitions with their spread.  No bar: the ratio is reported.

    python tools/gpu_swd_ellip_perf.py [--out profiles/swd_ellip_perf.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--layers", type=int, default=10)
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from bayhunter_amd import engine as E
    from bayhunter_amd.synth import SEED, SWD_PERIODS, synth_models
    eng = E.default_engine(0)
    dev = torch.device("cuda", eng.device)
    B, L, K = a.batch, a.layers, SWD_PERIODS.size
    nlay, h, vp, vs, rho = synth_models(np.random.RandomState(SEED), B, L, lvz_frac=0.1)
    t = {k: torch.as_tensor(v, device=dev) for k, v in dict(nlay=nlay, h=h, vp=vp, vs=vs, rho=rho, per=SWD_PERIODS).items()}
    vel = torch.zeros((B, K), dtype=torch.float64, device=dev)
    err = torch.zeros(B, dtype=torch.int32, device=dev)
    hv, mis, cpol = (torch.zeros((B, K), dtype=torch.float64, device=dev) for _ in range(3))
    flag = torch.zeros(B, dtype=torch.int32, device=dev)
    model = (B, L, t["nlay"].data_ptr(), t["h"].data_ptr(), t["vp"].data_ptr(), t["vs"].data_ptr(), t["rho"].data_ptr(), B, 1, K,
             t["per"].data_ptr())

    def fence():
        torch.cuda.synchronize(dev)
        eng.synchronize()

    def search():
        eng.swd_batch_dev(*model, E.WAVE_RAYLEIGH, E.VEL_PHASE, vel.data_ptr(), err.data_ptr())

    def ellip(nsteps):
        eng.swd_ellip_dev(*model, vel.data_ptr(), err.data_ptr(), hv.data_ptr(), flag.data_ptr(), have_vel=True, nsteps=nsteps,
                          mismatch=mis.data_ptr(), cpol=cpol.data_ptr())

    def timed(fn):
        fence()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            fn()
        fence()
        return (time.perf_counter() - t0) / a.calls * 1e3

    search(); ellip(2); ellip(0)     # (untimed: first launches)
    fence()
    ms = {"S": [], "E": [], "E0": []}
    for rep in range(a.reps):
        for name in (("S", "E", "E0") if rep % 2 == 0 else ("E0", "E", "S")):
            ms[name].append(timed(search if name == "S" else (lambda: ellip(2)) if name == "E" else (lambda: ellip(0))))
    ellip(2)
    fence()
    ok = (err.cpu().numpy() == 0)
    m = mis.cpu().numpy()[ok]
    res = dict(workload="%d models x %d layers (bayhunter_amd.synth.synth_models, lvz_frac 0.1), %d periods; device arrays, %d calls per "
                        "timing, best of %d" % (B, L, K, a.calls, a.reps),
               search=dict(search=eng.swd_search(), arith=eng.swd_arith()),
               ms_per_call={k: dict(best=min(v), all=v, spread=max(v) - min(v)) for k, v in ms.items()},
               ellip_over_search=min(ms["E"]) / min(ms["S"]), ellip0_over_search=min(ms["E0"]) / min(ms["S"]),
               pairs_per_s_ellip=B * K / (min(ms["E"]) * 1e-3),
               models_failed=int((~ok).sum()), models_flagged=int((flag.cpu().numpy() != 0).sum()),
               mismatch_after_polish=dict(max=float(m.max()), median=float(np.median(m))), bar=None)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
