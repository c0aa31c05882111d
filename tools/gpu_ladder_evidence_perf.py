"""Evidence estimates of tempered runs: time of the engine call behind diagnostics.ladder_evidence on the workload of
tools/gpu_chain_diag_ladders_perf.py -- synthetic AR(1) likes and betas that lie on the device as record="device" leaves them, the
betas permuted inside every ladder at every --permute-every'th row.  Two routes in one session, best of --reps with the spread:

  A  diagnostics.ladder_evidence_sums: bh_chain_ladder_evidence, the holders of every rung and the four sums per rung series, the
     tables read where they lie; the stepping-stone sums `ss` from them on the host
  B  what a user has without a host copy and without the call: torch.argsort of every row's betas per ladder, torch.take_along_dim
     of the likes, torch.exp, sum, and `ss` from those (float64 on the device, the device library's exp)

The bar: A is no slower than B by more than the spread of B's repeats.  The largest |A - B| of `ss` is reported.  --trace N: N calls
of each route and nothing else, for one `rocprofv3 --kernel-trace --stats` run (per-kernel times are not taken otherwise).

    python tools/gpu_ladder_evidence_perf.py [--sites 64] [--ladders 2] [--temps 4] [--rows 20000] [--out profiles/ladder_evidence_perf.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=64)
    ap.add_argument("--ladders", type=int, default=2)
    ap.add_argument("--temps", type=int, default=4)
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--permute-every", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from bayhunter_amd import diagnostics as D
    from bayhunter_amd import engine as E
    from gpu_chain_diag_perf import ar1
    from gpu_chain_diag_ladders_perf import permuted_betas, timed
    eng = E.default_engine(0)
    dev = torch.device("cuda", 0)
    T, R = a.rows, a.temps
    K = a.sites * a.ladders
    Cn = K * R
    ladder = np.arange(Cn) // R
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    likes = (-1e4 + 3.0 * ar1(torch, (T, Cn), 0.9, dev, gen)).to(torch.float32)
    beta = permuted_betas(torch, T, ladder, a.permute_every, dev)
    sync = lambda: torch.cuda.synchronize(dev)
    sync()

    def route_a():
        s = D.ladder_evidence_sums(beta, likes, ladder, engine=eng)
        rb = s["rung_beta"].reshape(K, R)
        d = rb[:, :-1] - rb[:, 1:]
        return (np.log(s["sf"].reshape(K, R)[:, 1:] / T) + d * s["mx"].reshape(K, R)[:, 1:]).sum(axis=1)

    def route_b():
        b3 = beta.view(T, K, R)
        order = torch.argsort(b3, dim=2, descending=True)
        l3 = torch.take_along_dim(likes.view(T, K, R).double(), order, 2)           # [T][K][R]: the rung series
        rb = torch.take_along_dim(b3[0], order[0], 1)                               # [K][R]
        d = rb[:, :-1] - rb[:, 1:]                                                   # [K][R-1]: the step from rung r + 1 to rung r
        hot = l3[:, :, 1:]
        mx = hot.amax(dim=0)
        sf = torch.exp(d[None] * (hot - mx[None])).sum(dim=0)
        return (torch.log(sf / T) + d * mx).sum(dim=1).cpu().numpy()

    # warm-up (code objects, allocations)
    D.ladder_evidence_sums(beta[:64, :R], likes[:64, :R], ladder[:R], engine=eng)
    route_b()
    sync()
    if a.trace:
        for _ in range(a.trace):
            route_a()
        for _ in range(a.trace):
            route_b()
        sync()
        return
    ss_a, t_a = timed(route_a, a.reps, sync)
    ss_b, t_b = timed(route_b, a.reps, sync)
    res = dict(sites=a.sites, ladders_per_site=a.ladders, temperatures=R, chains=Cn, rows=T, permute_every=a.permute_every, dtype="float32",
               route_a=t_a, route_a_note="bh_chain_ladder_evidence on the [T][%d] tables where they lie: holders + extremes + sums" % Cn,
               route_b=t_b, route_b_note="torch.argsort per ladder and row + take_along_dim + exp + sum, float64 on the device",
               a_over_b=t_a["best_s"] / t_b["best_s"], max_abs_ss_a_minus_b=float(np.max(np.abs(ss_a - ss_b))),
               ss_range=[float(ss_a.min()), float(ss_a.max())],
               bar="A no slower than B by more than the spread of B's repeats",
               bar_met=bool(t_a["best_s"] <= t_b["best_s"] + t_b["spread_s"]),
               per_kernel_times="profiles/ladder_evidence_kernels.txt (one kernel trace, a run of its own)")
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
