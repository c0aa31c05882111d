"""Covariance of vs with depth: the time of posterior_covariance on the workload of tools/gpu_posterior_perf.py (S sites x N float32
models, the default 201 depths), best of three with the spread of the three, all in one session.  The rows are on the device for
every route.

  A  posterior_covariance(rows, site): mean, covariance and correlation of the 201 depth columns of every site
  B  what a user has today without a host copy: per site the vs-at-depth table formed with torch operations on the device
     (tools/gpu_posterior_quantiles_perf.torch_table), widened to float64, centred, V^T @ V / N in float64
  C  A with the Moho depth and the mean crustal vs beside the 201 depths (203 columns; rows without a Moho are left out)

The bar: A is no slower than B by more than the spread of B's repeats.  Also recorded: how close B's floating-point result comes
to A's exact one (the largest difference relative to the entry, and relative to sqrt(cov_ii cov_jj)).

    python tools/gpu_posterior_cov_perf.py [--sites 64] [--models 200000] [--out profiles/posterior_cov_perf.json]

Per-kernel times: `rocprofv3 --kernel-trace --stats -- python tools/gpu_posterior_cov_perf.py --only-a --reps 1`.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def torch_cov(rows, S, N, dep):
    """route B: cov [S, D, D] float64 on the host; rows [S * N, 2*ML] grouped by site, N rows each"""
    import torch
    from gpu_posterior_quantiles_perf import torch_table
    D = dep.numel()
    out = torch.empty((S, D, D), dtype=torch.float64, device=rows.device)
    for s in range(S):                                       # (site by site: the intermediates of one site at a time)
        v = torch_table(rows[s * N:(s + 1) * N], dep).to(torch.float64)
        v -= v.mean(0, keepdim=True)
        out[s] = (v.T @ v) / N
        del v
    return out.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=64)
    ap.add_argument("--models", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only-a", action="store_true", help="route A alone (for a per-kernel trace)")
    ap.add_argument("--commit", default=None, help="the commit measured (default: git's HEAD)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from bayhunter_amd import engine as E
    from bayhunter_amd.posterior import default_dep_int, posterior_covariance
    from gpu_posterior_perf import rows as make_rows
    from gpu_posterior_quantiles_perf import commit, timed
    eng = E.Engine(0)
    rs = np.random.RandomState(1)
    S, N = a.sites, a.models
    dep = default_dep_int()
    m = torch.from_numpy(make_rows(rs, S * N)).cuda()
    site = torch.arange(S, dtype=torch.int32, device=m.device).repeat_interleave(N)
    dep_t = torch.from_numpy(dep).cuda()

    def route_a(**kw):
        r = posterior_covariance(m, site=site, engine=eng, nsites=S, **kw)
        torch.cuda.synchronize()
        return r

    def route_b():
        v = torch_cov(m, S, N, dep_t)
        torch.cuda.synchronize()
        return v

    ra = route_a()                                           # (the warm-up as well)
    ca = np.stack([r["cov"] for r in ra])
    assert ca.shape == (S, dep.size, dep.size) and all(r["n"] == N and r["exact"].all() for r in ra)
    _, t_a = timed(route_a, a.reps)
    res = dict(commit=a.commit or commit(), device=torch.cuda.get_device_name(0), sites=S, models_per_site=N, depths=int(dep.size),
               dtype="float32", layers="1-21", reps=a.reps, rows="on the device for every route", A_posterior_covariance=t_a)
    if not a.only_a:
        cb = route_b()
        scale = np.sqrt(np.einsum("sii,sjj->sij", ca, ca))
        nz = ca != 0
        res.update(B_largest_difference_relative_to_the_entry=float(np.max(np.abs(cb - ca)[nz] / np.abs(ca[nz]))),
                   B_largest_difference_relative_to_sqrt_cii_cjj=float(np.max(np.abs(cb - ca)[scale > 0] / scale[scale > 0])))
        _, t_b = timed(route_b, a.reps)
        moho = dict(moho=(10.0, 60.0), mohovs=4.2)
        rc = route_a(**moho)
        _, t_c = timed(lambda: route_a(**moho), a.reps)
        res.update(B_torch_table_centred_matmul_float64=t_b, C_with_moho_and_vscrust=t_c,
                   C_rows_used_of_site_0=int(rc[0]["n"]), C_columns=len(rc[0]["names"]),
                   bar="A_posterior_covariance.best_s <= B.best_s + B.spread_s",
                   bar_met=bool(t_a["best_s"] <= t_b["best_s"] + t_b["spread_s"]))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
