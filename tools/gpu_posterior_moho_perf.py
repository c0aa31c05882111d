"""Moho and scalar posteriors of many sites: time of one posterior_moho call (and one posterior_scalars call with two
columns) on S sites x N float32 models, from host rows (the host->device copy of the rows included) and from device rows,
best of --reps with the spread.  Beside it two baselines: the numpy restatement (tests/moho_ref.py) on the rows of one
site, timed in the same session on --ref-rows rows and scaled linearly to N; and the reference's own loop over the
posterior models (plot_moho_crustvel_tradeoff), whose seconds per 10 000 rows tests/golden/gen_moho_golden.py measured on the
build machine's CPU and stored in tests/golden/moho_golden.npz -- another machine and another session, so an estimate.

    python tools/gpu_posterior_moho_perf.py [--sites 64] [--models 200000] [--out profiles/posterior_moho_perf.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def rows(rs, N, ML=21):
    """a slow crust over a fast mantle, 2-21 layers"""
    base = np.full((65536, 2 * ML), np.nan, np.float32)
    for i in range(len(base)):
        n = rs.randint(2, ML + 1)
        nc = rs.randint(1, n)
        base[i, :n] = np.concatenate((rs.uniform(2.0, 4.1, nc), rs.uniform(3.9, 4.8, n - nc)))
        base[i, n:2 * n] = np.sort(rs.uniform(0, 60, n))
    return base[rs.randint(0, len(base), N)]


def timed(fn, reps):
    out, times = None, []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t)
    return out, dict(best_s=min(times), all_s=times, spread_s=max(times) - min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=64)
    ap.add_argument("--models", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref-rows", type=int, default=20000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from bayhunter_amd import engine as E
    from bayhunter_amd.posterior import posterior_moho, posterior_scalars
    import moho_ref as MR
    eng = E.Engine(0)
    rs = np.random.RandomState(1)
    S, N = a.sites, a.models
    m = rows(rs, S * N)
    site = np.repeat(np.arange(S, dtype=np.int32), N)
    likes = rs.normal(800, 10, S * N).astype(np.float32)
    vpvs = rs.uniform(1.4, 2.1, S * N).astype(np.float32)
    moho = np.stack((rs.uniform(0, 10, S), rs.uniform(40, 60, S)), axis=1)
    mv = rs.uniform(4.0, 4.3, S)
    posterior_moho(m[:4096], site=site[:4096] * 0, moho=(5.0, 50.0), engine=eng)        # warm-up (code objects, allocations)
    posterior_scalars(m[:4096], dict(likes=likes[:4096]), site=site[:4096] * 0, engine=eng)
    r_host, t_host = timed(lambda: posterior_moho(m, site=site, moho=moho, mohovs=mv, engine=eng), a.reps)
    _, ts_host = timed(lambda: posterior_scalars(m, dict(likes=likes, vpvs=vpvs), site=site, engine=eng), a.reps)
    md, sd = torch.from_numpy(m).cuda(), torch.from_numpy(site).cuda()
    ld, vd = torch.from_numpy(likes).cuda(), torch.from_numpy(vpvs).cuda()
    torch.cuda.synchronize()
    r_dev, t_dev = timed(lambda: posterior_moho(md, site=sd, moho=moho, mohovs=mv, engine=eng, nsites=S), a.reps)
    _, ts_dev = timed(lambda: posterior_scalars(md, dict(likes=ld, vpvs=vd), site=sd, engine=eng, nsites=S), a.reps)
    same = all(r_host[s]["count"] == r_dev[s]["count"] and r_host[s]["moho"] == r_dev[s]["moho"] for s in range(S))
    nref = min(a.ref_rows, N)
    t = time.perf_counter()
    ref = MR.moho_summary(m[:nref], moho[0, 0], moho[0, 1], mv[0])
    t_np = (time.perf_counter() - t) * N / nref
    g = np.load(os.path.join(ROOT, "tests", "golden", "moho_golden.npz"))
    t_ref = float(g["ref_loop_seconds_per_10000_rows"]) * N / 1e4
    res = dict(sites=S, models_per_site=N, dtype="float32", layers="2-21", bins=50,
               moho_from_host_rows=t_host, moho_from_device_rows=t_dev,
               scalars_2_columns_from_host_rows=ts_host, scalars_2_columns_from_device_rows=ts_dev,
               restatement_numpy_s_one_site_est=t_np, restatement_rows_timed=nref,
               restatement_numpy_s_all_sites_est=t_np * S,
               reference_loop_s_one_site_est=t_ref, reference_loop_s_all_sites_est=t_ref * S,
               reference_loop_note="plot_moho_crustvel_tradeoff's loop, measured on the build machine's CPU (tests/golden/"
                                   "moho_golden.npz), scaled linearly: not this machine, not this session",
               rows_with_a_moho_site0=int(r_host[0]["count"]), host_and_device_agree=bool(same),
               restatement_count_first_rows=int(ref["count"]))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
