"""Rank-normalised diagnostics of many sites: the time of diagnose(rank=True) on the synthetic tables of tools/gpu_chain_diag_perf.py
(on the device as record="device" leaves them), one session, the same tensors for every route, a warm-up, best of --reps with the
spread:

  A  diagnose(rank=True); and its rank stage alone -- the rank_series / rank_models calls of rank_convergence, in its chunks,
     without the sums that follow.
  B  the same numbers with the rank tables formed by what torch offers today: the vs-at-depth table with torch operations, per
     column one torch.sort over every pool (a batched sort along the pool axis), the tie runs with torch.unique_consecutive, the
     same zt lookup; then the same chain_series_stats and convergence.  Its rank stage is timed alone as well, with and without the
     forming of the vs table.
  C  diagnose() without ranks: the floor of the shared part.

The bar: the rank stage of A is no slower than B's by more than the spread of B's repeats; A and B agree bit for bit.  Also: the
rank stage's rate in keys per second and pass (a pass of the radix sort moves every key once), its share of A, and a float64 copy of
one float32 table through the same calls -- 8 passes of 64-bit keys instead of 4 of 32-bit: what the 32-bit path of float32 tables
buys.

    python tools/gpu_chain_rank_perf.py [--sites 64] [--chains 8] [--rows 20000] [--out profiles/chain_rank_perf.json]
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

from gpu_chain_diag_perf import tables  # noqa: E402


def vs_table_torch(torch, models, dep, rows=250):
    """torch: vs at dep and nlayers [T][C][D+1] (float64) of model rows [T][C][2ML] (the rule of posterior_models), in row chunks"""
    T, Cn, W = models.shape
    ML = W // 2
    dev = models.device
    out = torch.empty((T, Cn, dep.numel() + 1), dtype=torch.float64, device=dev)
    j = torch.arange(ML, device=dev)
    for r0 in range(0, T, rows):
        m = models[r0:r0 + rows]
        n = (~torch.isnan(m)).sum(dim=2) // 2
        vs = torch.gather(m, 2, torch.minimum(j.expand_as(m[..., :ML]), (n - 1)[..., None]))
        z = torch.gather(m, 2, torch.minimum(n[..., None] + j, (2 * n - 1)[..., None]))
        zd = ((z[..., :-1] + z[..., 1:]) / 2).to(torch.float64)
        h = torch.diff(torch.cat((torch.zeros_like(zd[..., :1]), zd), dim=2), dim=2)
        d = torch.cumsum(h, dim=2)
        d = torch.where(j[:-1] >= (n - 1)[..., None], torch.full_like(d, float("inf")), d)
        k = (d[..., :, None] <= dep).sum(dim=2)
        out[r0:r0 + rows, :, :-1] = torch.gather(vs, 2, k).to(torch.float64)
        out[r0:r0 + rows, :, -1] = (n - 1).to(torch.float64)
    return out


def torch_scores(torch, pools, zt):
    """normal scores of pools [G][N] (float64, -0.0 already +0.0), each row ranked on its own: torch.sort along the row, the tie
    runs of the sorted rows with torch.unique_consecutive, R2 = 2 lt + eq + 1, zt[R2] back at the elements' places; and lt"""
    G, N = pools.shape
    srt, idx = torch.sort(pools, dim=1)
    head = torch.ones((G, N), dtype=torch.bool, device=pools.device)
    head[:, 1:] = srt[:, 1:] != srt[:, :-1]
    run = torch.cumsum(head.reshape(-1), 0)
    _, cnt = torch.unique_consecutive(run, return_counts=True)
    start = torch.cumsum(cnt, 0) - cnt
    lt = torch.repeat_interleave(start, cnt).reshape(G, N) - (torch.arange(G, device=pools.device) * N)[:, None]
    eq = torch.repeat_interleave(cnt, cnt).reshape(G, N)
    z = torch.empty_like(pools)
    z.scatter_(1, idx, zt[2 * lt + eq + 1])
    ltx = torch.empty_like(lt)
    ltx.scatter_(1, idx, lt)
    return z, ltx, srt


def torch_rank_tables(torch, x, sites, zt):
    """z, zf, tail of x [T][C][Q] with the chains of site s at sites[s] (all of one size), column by column"""
    T, Cn, Q = x.shape
    G, m = sites.shape
    N = T * m
    z = torch.zeros((T, Cn, Q), dtype=torch.float64, device=x.device)
    zf = torch.zeros_like(z)
    tail = torch.zeros((T, Cn, 2 * Q), dtype=torch.float32, device=x.device)
    flat = sites.reshape(-1)
    for q in range(Q):
        v = x[:, flat, q].to(torch.float64).reshape(T, G, m).permute(1, 0, 2).reshape(G, N) + 0.0
        a, lt, srt = torch_scores(torch, v, zt)
        med = (srt[:, (N - 1) // 2] + srt[:, N // 2]) * 0.5
        b, _, _ = torch_scores(torch, (v - med[:, None]).abs(), zt)
        back = lambda t: t.reshape(G, T, m).permute(1, 0, 2).reshape(T, G * m)       # noqa: E731
        z[:, flat, q], zf[:, flat, q] = back(a), back(b)
        tail[:, flat, 2 * q] = back((lt <= (N - 1) // 20).to(torch.float32))
        tail[:, flat, 2 * q + 1] = back((lt <= (19 * (N - 1)) // 20).to(torch.float32))
    return z, zf, tail


def timed(torch, fn, reps):
    out, times = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    return out, dict(best_s=min(times), all_s=times, spread_s=max(times) - min(times))


def same(a, b):
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
    x, y = np.asarray(a), np.asarray(b)
    return x.shape == y.shape and bool(np.array_equal(x, y, equal_nan=(x.dtype.kind == "f")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=64)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--rows", type=int, default=20000)
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
    eng = E.default_engine(0)
    dev = torch.device("cuda", 0)
    S, Cs, T, L = a.sites, a.chains, a.rows, a.maxlag
    Cn = S * Cs
    dep = np.linspace(0, 100, a.depths)
    tdep = torch.from_numpy(dep).to(dev)
    tabs = tables(torch, T, Cn, a.nt, a.layers, dev)
    torch.cuda.synchronize()
    site_of, ids = np.arange(Cn) // Cs, np.arange(Cn)
    names = ("likes", "vpvs", "misfits", "noise")
    budget = 2 << 30
    step = int(max(1, min(E.DIAG_MAXCOLS, budget // (24 * T * Cn))))

    def chunks(Q):
        return [(q0, min(step, Q - q0)) for q0 in range(0, Q, step)]

    def route_a():
        return D.diagnose(tabs, site_of, ids, dep=dep, maxlag=L, engine=eng, rank=True)

    def route_c():
        return D.diagnose(tabs, site_of, ids, dep=dep, maxlag=L, engine=eng)

    def rank_stage_a():
        ex = exclude
        group = np.where(np.isin(ids, ex), -1, site_of)
        for k in names:
            v = tabs[k]
            for q0, nq in chunks(v.shape[2] if v.dim() == 3 else 1):
                D.rank_series(v if v.dim() == 2 else v[:, :, q0:q0 + nq], group, engine=eng)
        for q0, nq in chunks(dep.size + 1):
            D.rank_models(tabs["models"], dep, group, engine=eng, columns=(q0, nq))

    def b_tables(k, q0, nq, vt):
        v = vt if k == "models" else tabs[k]
        v = v[:, :, None] if v.dim() == 2 else v
        return torch_rank_tables(torch, v[:, :, q0:q0 + nq], sites, zt)

    def rank_stage_b(with_table=True):
        vt = vs_table_torch(torch, tabs["models"], tdep) if with_table else vtab
        for k in names:
            for q0, nq in chunks(tabs[k].shape[2] if tabs[k].dim() == 3 else 1):
                b_tables(k, q0, nq, None)
        for q0, nq in chunks(dep.size + 1):
            b_tables("models", q0, nq, vt)

    def route_b():
        out = route_c()
        vt = vs_table_torch(torch, tabs["models"], tdep)
        D_ = dep.size
        for k in names + ("models",):
            Q = D_ + 1 if k == "models" else (tabs[k].shape[2] if tabs[k].dim() == 3 else 1)
            parts = []
            for q0, nq in chunks(Q):
                conv = [D.convergence(D.chain_series_stats(t, L, engine=eng), site_of, exclude) for t in b_tables(k, q0, nq, vt)]
                parts.append([D.rank_summary(x, y, w) for x, y, w in zip(*conv)])
            for s in range(S):
                r = {f: (ids[parts[0][s][f]] if f == "chains" else np.concatenate([np.atleast_1d(p[s][f]) for p in parts]))
                     for f in ("chains",) + D.RANK_FIELDS}
                if k == "models":
                    out[s]["vs"]["rank"] = {f: (v if f == "chains" else v[..., :D_]) for f, v in r.items()}
                    out[s]["nlayers"]["rank"] = {f: (v if f == "chains" else v[..., D_]) for f, v in r.items()}
                else:
                    out[s][k]["rank"] = r
        return out

    # warm-up: code objects, allocator pools, the outliers that every route excludes
    small = {k: v[:64, :Cs] for k, v in tabs.items()}
    D.diagnose(small, site_of[:Cs], ids[:Cs], dep=dep, maxlag=8, engine=eng, rank=True)
    outl, _ = D.outlier_chains(tabs["likes"], site_of, engine=eng)
    exclude = np.concatenate(outl) if outl else np.zeros(0, np.int64)
    kept = ~np.isin(ids, exclude)
    per_site = [ids[(site_of == s) & kept] for s in range(S)]
    if len(set(len(p) for p in per_site)) != 1:
        raise SystemExit("route B batches the sort over pools of one size: the sites keep different numbers of chains here")
    sites = torch.from_numpy(np.stack(per_site)).to(dev)
    zt = torch.from_numpy(D.rank_table(T * sites.shape[1])).to(dev)
    vtab = vs_table_torch(torch, tabs["models"], tdep)
    torch.cuda.synchronize()

    _, t_c = timed(torch, route_c, a.reps)
    _, t_ra = timed(torch, rank_stage_a, a.reps)
    r_a, t_a = timed(torch, route_a, a.reps)
    _, t_rb = timed(torch, rank_stage_b, a.reps)
    _, t_rb0 = timed(torch, lambda: rank_stage_b(False), a.reps)
    _, t_vt = timed(torch, lambda: vs_table_torch(torch, tabs["models"], tdep), a.reps)
    r_b, t_b = timed(torch, route_b, 1)
    agree = all(same(r_a[s], r_b[s]) for s in range(S))
    differing = sorted({(k, f) for s in range(S) for k in D.GROUPS for f in D.RANK_FIELDS
                        if not same(r_a[s][k]["rank"][f], r_b[s][k]["rank"][f])})

    # 32-bit against 64-bit keys: the misfits table as it is and as float64
    group = np.where(np.isin(ids, exclude), -1, site_of)
    m32 = tabs["misfits"]
    m64 = m32.to(torch.float64)
    _, t_32 = timed(torch, lambda: D.rank_series(m32, group, engine=eng), a.reps)
    _, t_64 = timed(torch, lambda: D.rank_series(m64, group, engine=eng), a.reps)
    del m64

    cols = 2 + (a.nt + 1) + 2 * a.nt + a.depths + 1
    keys = int(kept.sum()) * T * cols
    passes = 4 + 8                      # float32 tables: 4 passes of 32-bit keys, then 8 of the 64-bit folded keys
    res = dict(sites=S, chains_per_site=Cs, rows=T, nt=a.nt, depths=a.depths, maxlag=L, layers_max=a.layers, dtype="float32",
               columns=cols, pools=S * cols, keys=keys, column_chunk=step,
               A_diagnose_rank=t_a, A_rank_stage=t_ra, B_torch_route=t_b, B_rank_stage=t_rb, B_rank_stage_without_vs_table=t_rb0,
               B_vs_table=t_vt, C_diagnose=t_c,
               bar="A_rank_stage.best_s <= B_rank_stage.best_s + B_rank_stage.spread_s",
               bar_met=bool(t_ra["best_s"] <= t_rb["best_s"] + t_rb["spread_s"]),
               bar_met_without_vs_table=bool(t_ra["best_s"] <= t_rb0["best_s"] + t_rb0["spread_s"]),
               A_and_B_agree_bit_for_bit=bool(agree), differing_fields=[list(d) for d in differing],
               rank_stage_share_of_A=t_ra["best_s"] / t_a["best_s"],
               keys_per_s_per_pass=keys * passes / t_ra["best_s"],
               rate_note="keys x (4 + 8) passes over the time of the whole rank stage of A (check, extract, sorts, tie runs, writes, "
                         "the zt uploads): a lower bound of the sort passes' own rate",
               misfits_float32_keys32=t_32, misfits_float64_keys64=t_64,
               key_width_note="rank_series of the misfits table [T][C][nt+1] as float32 (4 + 8 passes per column) and copied to "
                              "float64 (8 + 8 passes)")
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
