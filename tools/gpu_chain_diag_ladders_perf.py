"""Convergence diagnostics of tempered runs: time of the calls behind DeviceChains.ladder_diagnostics on synthetic AR(1) tables that lie
on the device as record="device" leaves them (the tables of tools/gpu_chain_diag_perf.py), with betas that are permuted inside every
ladder at every --permute-every'th row.  Three routes in one session, best of --reps with the spread:

  A  ladder_index, then diagnose(sel=) on the [T][C] tables: the cold series are read where the rows lie
  B  what a user could do on the device before: ladder_index's selection, every table gathered to [T][K][..] with torch indexing, then
     diagnose() on the gathered tables (a second copy of the cold rows)
  C  diagnose() on tables gathered beforehand, the copy not timed: the kernels' floor

The bar: A is no slower than B by more than the spread of B's repeats.  A / C is reported, not gated.  Per-kernel times are not taken
here ("unmeasured"): that needs a kernel trace in a run of its own.

    python tools/gpu_chain_diag_ladders_perf.py [--sites 64] [--ladders 2] [--temps 4] [--rows 20000] [--out profiles/chain_diag_ladders_perf.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def permuted_betas(torch, T, ladder, every, dev):
    """float64 [T][C]: every ladder's geometric temperatures, permuted anew at every `every`'th row"""
    C = ladder.size
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    beta = torch.empty((T, C), dtype=torch.float64, device=dev)
    nblk = (T + every - 1) // every
    for lid in np.unique(ladder):
        idx = torch.from_numpy(np.flatnonzero(ladder == lid)).to(dev)
        n = idx.numel()
        b = torch.from_numpy(1.0 / np.geomspace(1.0, 20.0, n) if n > 1 else np.ones(1)).to(dev)
        perm = torch.argsort(torch.rand((nblk, n), device=dev, generator=gen), dim=1)          # [blocks][n]
        beta[:, idx] = b[perm].repeat_interleave(every, dim=0)[:T]
    return beta


def timed(fn, reps, sync):
    out, times = None, []
    for _ in range(reps):
        sync()
        t = time.perf_counter()
        out = fn()
        sync()
        times.append(time.perf_counter() - t)
    return out, dict(best_s=min(times), all_s=times, spread_s=max(times) - min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=64)
    ap.add_argument("--ladders", type=int, default=2)
    ap.add_argument("--temps", type=int, default=4)
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--permute-every", type=int, default=5)
    ap.add_argument("--nt", type=int, default=3)
    ap.add_argument("--depths", type=int, default=41)
    ap.add_argument("--maxlag", type=int, default=1000)
    ap.add_argument("--layers", type=int, default=21)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from bayhunter_amd import diagnostics as D
    from bayhunter_amd import engine as E
    from gpu_chain_diag_perf import tables
    eng = E.default_engine(0)
    dev = torch.device("cuda", 0)
    S, T, L = a.sites, a.rows, a.maxlag
    Cs = a.ladders * a.temps
    Cn, K = S * Cs, S * a.ladders
    dep = np.linspace(0, 100, a.depths)
    ladder = np.arange(Cn) // a.temps
    site_of_ladder, ids = np.arange(K) // a.ladders, np.arange(K)
    tabs = tables(torch, T, Cn, a.nt, a.layers, dev)
    tabs["beta"] = permuted_betas(torch, T, ladder, a.permute_every, dev)
    sync = lambda: torch.cuda.synchronize(dev)
    sync()
    names = ("likes", "vpvs", "misfits", "noise", "models")

    def gather(sel):
        idx = sel.long()
        rows = torch.arange(T, device=dev)[:, None]
        return {k: tabs[k][rows, idx] for k in names}

    def route_a():
        idx = D.ladder_index(tabs["beta"], ladder, engine=eng)
        return idx, D.diagnose(tabs, site_of_ladder, ids, dep=dep, maxlag=L, engine=eng, sel=idx["sel"])

    def route_b():
        idx = D.ladder_index(tabs["beta"], ladder, engine=eng)
        return D.diagnose(gather(idx["sel"]), site_of_ladder, ids, dep=dep, maxlag=L, engine=eng)

    # warm-up (code objects, allocations)
    small = {k: v[:64, :Cs] for k, v in tabs.items()}
    i0 = D.ladder_index(small["beta"], ladder[:Cs], engine=eng)
    D.diagnose(small, site_of_ladder[:a.ladders], ids[:a.ladders], dep=dep, maxlag=8, engine=eng, sel=i0["sel"])
    D.diagnose({k: v[:64, :a.ladders] for k, v in tabs.items() if k != "beta"}, site_of_ladder[:a.ladders], ids[:a.ladders], dep=dep, maxlag=8,
               engine=eng)
    (idx, r_a), t_a = timed(route_a, a.reps, sync)
    r_b, t_b = timed(route_b, a.reps, sync)
    pre = gather(idx["sel"])
    sync()
    r_c, t_c = timed(lambda: D.diagnose(pre, site_of_ladder, ids, dep=dep, maxlag=L, engine=eng), a.reps, sync)
    _, t_i = timed(lambda: D.ladder_index(tabs["beta"], ladder, engine=eng), a.reps, sync)

    def equal(x, y):
        return all(np.array_equal(x[s][g][k], y[s][g][k], equal_nan=True) for s in range(S) for g in D.GROUPS for k in ("rhat", "ess", "tau", "mean"))
    res = dict(sites=S, ladders_per_site=a.ladders, temperatures=a.temps, chains=Cn, series_per_table=K, rows=T, permute_every=a.permute_every,
               nt=a.nt, depths=a.depths, maxlag=L, layers_max=a.layers, dtype="float32",
               series=K * (2 + a.nt + 1 + 2 * a.nt + a.depths + 1), cold_moves_total=int(idx["moves"].sum()),
               route_a=t_a, route_a_note="ladder_index + diagnose(sel=) on the [T][%d] tables where they lie" % Cn,
               route_b=t_b, route_b_note="ladder_index + every table gathered to [T][%d][..] with torch indexing + diagnose()" % K,
               route_c=t_c, route_c_note="diagnose() on tables gathered beforehand (the copy not timed): the kernels' floor",
               ladder_index=t_i, ladder_index_share_of_a=t_i["best_s"] / t_a["best_s"],
               a_over_b=t_a["best_s"] / t_b["best_s"], a_over_c=t_a["best_s"] / t_c["best_s"],
               bar="A no slower than B by more than the spread of B's repeats",
               bar_met=bool(t_a["best_s"] <= t_b["best_s"] + t_b["spread_s"]),
               same_results_a_b_c=bool(equal(r_a, r_b) and equal(r_a, r_c)),
               per_kernel_times="unmeasured (no kernel trace was taken)")
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
