"""Credible bands of vs against depth: the time of the quantile stage of posterior_models(quantiles=...) on the workload of
tools/gpu_posterior_perf.py (S sites x N float32 models, the default 201 depths, the five quantiles 0.025 / 0.16 / 0.5 / 0.84 /
0.975), best of three with the spread of the three, all in one session.  The rows are on the device for every route.

  A  posterior_models(quantiles=Q) and posterior_models() -- the difference is the quantile stage; and the stage on its own
     (the five passes of bh_posterior_column_quantiles on a loaded handle with the finalisation in numpy)
  B  what a user has today without a host copy: per group of sites that fits the memory budget the vs-at-depth table formed with
     torch operations on the device (float32, [sites, rows, depths]), torch.sort along the rows, the 2R order statistics picked
     and the same interpolation
  C  one R = 5 call of bh_posterior_column_quantiles against five R = 1 calls: what the shared read buys

The bar: A's quantile stage is no slower than B by more than the spread of B's repeats.  A and B must agree bit for bit before
anything is timed.

    python tools/gpu_posterior_quantiles_perf.py [--sites 64] [--models 200000] [--out profiles/posterior_quantiles_perf.json]

Per-kernel times: `rocprofv3 --kernel-trace --stats -- python tools/gpu_posterior_quantiles_perf.py --reps 1`.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

QUANTILES = (0.025, 0.16, 0.5, 0.84, 0.975)


def torch_table(rows, dep):
    """vs of every row at every depth with torch operations: rows [N, 2*ML] (the reference's layout, every row valid), dep [D]
    float64 -> [N, D] in the rows' dtype.  The interface depths as the kernels form them: zd_j = (z_j + z_{j+1}) / 2 in the rows'
    dtype, d_j = the running float64 sum of zd_j - zd_{j-1}; vs at x = vs[#{d_j <= x}]."""
    import torch
    N, W = rows.shape
    ML = W // 2
    n = (~torch.isnan(rows)).sum(1) // 2
    cols = torch.arange(ML, device=rows.device)
    z = rows.gather(1, (n[:, None] + cols[None, :]).clamp(max=W - 1))
    zd = ((z[:, :-1] + z[:, 1:]) / 2).to(torch.float64)
    d = torch.empty_like(zd)
    run = torch.zeros(N, dtype=torch.float64, device=rows.device)
    prev = torch.zeros_like(run)
    for j in range(ML - 1):                                  # (a sequential sum, as numpy.cumsum and the kernel round it)
        run = run + (zd[:, j] - prev) if j else zd[:, j] - prev
        prev = zd[:, j]
        d[:, j] = run
    d = torch.where(cols[None, :-1] < (n - 1)[:, None], d, torch.full_like(d, float("inf")))
    k = torch.searchsorted(d, dep[None, :].expand(N, -1).contiguous(), right=True)
    return rows[:, :ML].gather(1, k)


def torch_quantiles(rows, S, N, dep, qs, budget):
    """route B: [S, R, D] float64 on the host; rows [S * N, 2*ML] grouped by site, N rows each"""
    import torch
    from bayhunter_amd.posterior import quantile_rank
    D = dep.numel()
    kg = [quantile_rank(N, q) for q in qs]
    lo = torch.tensor([k for k, _ in kg], device=rows.device)
    up = (lo + 1).clamp(max=N - 1)
    g = torch.tensor([v for _, v in kg], dtype=torch.float64, device=rows.device)[None, :, None]
    per = max(1, int(budget // (N * D * rows.element_size() * 5)))   # the table, its sorted copy and the int64 indices of torch.sort
    out = torch.empty((S, len(qs), D), dtype=torch.float64, device=rows.device)
    for s0 in range(0, S, per):
        s1 = min(S, s0 + per)
        tab = torch.empty((s1 - s0, N, D), dtype=rows.dtype, device=rows.device)
        for s in range(s0, s1):                              # (site by site: the intermediates of one site at a time)
            tab[s - s0] = torch_table(rows[s * N:(s + 1) * N], dep)
        srt = torch.sort(tab, dim=1).values
        a, b = srt[:, lo].to(torch.float64), srt[:, up].to(torch.float64)
        dd = b - a
        out[s0:s1] = torch.where(g >= 0.5, b - dd * (1.0 - g), a + dd * g)
        del tab, srt
    return out.cpu().numpy()


def timed(fn, reps):
    times, out = [], None
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t)
    return out, dict(best_s=min(times), all_s=times, spread_s=max(times) - min(times))


def commit():
    try:
        return subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=64)
    ap.add_argument("--models", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--budget-gib", type=float, default=16.0, help="device memory of one group of sites of route B")
    ap.add_argument("--commit", default=None, help="the commit measured (default: git's HEAD)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from bayhunter_amd import engine as E
    from bayhunter_amd.posterior import _Loaded, column_quantiles, default_dep_int, posterior_models, quantile_rank
    from gpu_posterior_perf import rows as make_rows
    eng = E.Engine(0)
    rs = np.random.RandomState(1)
    S, N = a.sites, a.models
    dep = default_dep_int()
    m = torch.from_numpy(make_rows(rs, S * N)).cuda()
    site = torch.arange(S, dtype=torch.int32, device=m.device).repeat_interleave(N)
    dep_t = torch.from_numpy(dep).cuda()
    budget = a.budget_gib * (1 << 30)

    def route_a(q):
        r = posterior_models(m, site=site, engine=eng, nsites=S, quantiles=q)
        torch.cuda.synchronize()
        return r

    def route_b():
        v = torch_quantiles(m, S, N, dep_t, QUANTILES, budget)
        torch.cuda.synchronize()
        return v

    # agreement first (this is the warm-up of both routes as well)
    ra = route_a(QUANTILES)
    vb = route_b()
    va = np.stack([r["quantiles"][0] for r in ra])
    assert va.shape == vb.shape == (S, len(QUANTILES), dep.size)
    assert np.array_equal(va.view(np.uint64), vb.view(np.uint64)), "routes A and B differ"
    route_a(None)

    _, t_aq = timed(lambda: route_a(QUANTILES), a.reps)
    _, t_a0 = timed(lambda: route_a(None), a.reps)
    _, t_b = timed(route_b, a.reps)
    ld = _Loaded(m, site, eng, S)
    try:
        _, t_stage = timed(lambda: column_quantiles(ld, dep, QUANTILES), a.reps)
        rank = np.array([[quantile_rank(N, q)[0] for q in QUANTILES]] * S, np.uint32)
        many, t_c5 = timed(lambda: ld.column_quantile_keys(dep, rank), a.reps)
        single, t_c1 = timed(lambda: [ld.column_quantile_keys(dep, rank[:, r:r + 1]) for r in range(rank.shape[1])], a.reps)
        for r in range(rank.shape[1]):
            assert np.array_equal(many[0][:, :, r], single[r][0][:, :, 0]) and np.array_equal(many[1][:, :, r], single[r][1][:, :, 0])
    finally:
        ld.close()
    stage = t_aq["best_s"] - t_a0["best_s"]
    res = dict(commit=a.commit or commit(), device=torch.cuda.get_device_name(0), sites=S, models_per_site=N, depths=int(dep.size),
               dtype="float32", layers="1-21", quantiles=list(QUANTILES), reps=a.reps, rows="on the device for every route",
               A_with_quantiles=t_aq, A_without_quantiles=t_a0, A_quantile_stage_by_difference_s=stage,
               A_quantile_stage_alone=t_stage, B_torch_sort=t_b, B_budget_gib=a.budget_gib,
               C_one_call_of_5_ranks=t_c5, C_five_calls_of_1_rank=t_c1,
               C_shared_read_speedup=t_c1["best_s"] / t_c5["best_s"],
               agree_bit_for_bit=True,
               bar="A_quantile_stage_by_difference_s <= B_torch_sort.best_s + B_torch_sort.spread_s",
               bar_met=bool(stage <= t_b["best_s"] + t_b["spread_s"]),
               per_kernel="per-kernel times are unmeasured")
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
