"""Posterior summaries of many sites: time of one posterior_models call on S sites x N float32 models x 201 depths
(0.5 km, the default grid), including the host->device copy of the rows, against the vectorised numpy restatement
(tests/posterior_ref.py) on one site and the reference's get_singlemodels time measured on one CPU core (1.35 s per
20 000 models of 1-21 layers, numpy 2.2; it scales linearly with the models).

    python tools/gpu_posterior_perf.py [--sites 64] [--models 200000] [--out profiles/posterior_perf.json]

Per-kernel times: `rocprofv3 --kernel-trace --stats -- python tools/gpu_posterior_perf.py --sites 64 --models 200000 --reps 1`.
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

REF_S_PER_MODEL = 1.35 / 20000


def rows(rs, N, ML=21):
    base = np.full((65536, 2 * ML), np.nan, np.float32)
    n = rs.randint(1, ML + 1, len(base))
    for i in range(len(base)):
        base[i, :n[i]] = rs.uniform(2.0, 4.8, n[i])
        base[i, n[i]:2 * n[i]] = np.sort(rs.uniform(0, 60, n[i]))
    return base[rs.randint(0, len(base), N)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=64)
    ap.add_argument("--models", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from bayhunter_amd import engine as E
    from bayhunter_amd.posterior import posterior_models
    import posterior_ref as R
    eng = E.Engine(0)
    rs = np.random.RandomState(1)
    S, N = a.sites, a.models
    m = rows(rs, S * N)
    site = np.repeat(np.arange(S, dtype=np.int32), N)
    posterior_models(m[:4096], site=site[:4096] * 0, engine=eng)        # warm-up (code objects, allocations)
    times = []
    for _ in range(a.reps):
        t = time.perf_counter()
        r = posterior_models(m, site=site, engine=eng)
        times.append(time.perf_counter() - t)
    t = time.perf_counter()
    R.singlemodels(m[:N], np.linspace(0, 100, 201))
    t_np = time.perf_counter() - t
    res = dict(sites=S, models_per_site=N, depths=201, dtype="float32", layers="1-21",
               gpu_s=min(times), gpu_s_all=times, restatement_numpy_s_one_site=t_np,
               restatement_numpy_s_all_sites_est=t_np * S,
               reference_s_per_site_est=REF_S_PER_MODEL * N, reference_s_all_sites_est=REF_S_PER_MODEL * N * S,
               speedup_vs_reference_est=REF_S_PER_MODEL * N * S / min(times),
               checked_count=int(r[0]["count"]))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
