"""Posterior data fits of many sites: time of one posterior_datafits call (bands at the default five quantiles and the best
fit of every chain) on S sites x N float32 rows, Rayleigh phase at 30 periods + a P receiver function, prior-like rows of
2-21 layers, with the engine's default search and arithmetic.  From host rows (the copies included) and from device rows,
best of --reps with the spread, and split into load, best, layers, forward, fill, statistics, quantiles and host work (the
split run drains the device after every phase, so its total is above the plain call's).

The baseline is what the package offered before for the same numbers, on --base-sites sites, SCALED linearly to S and stated
as scaled: Model.pack_batch on the host, the host evaluate_batch(want_ymod=True), numpy.quantile per site.

For the radix select: R ranks of every column in one multi-rank call against R single-rank calls of the same kernel.

    python tools/gpu_posterior_datafits_perf.py [--sites 64] [--models 8192] [--out profiles/posterior_datafits_perf.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ML = 21


def rows(rs, N):
    base = np.full((32768, 2 * ML), np.nan, np.float32)
    for i in range(len(base)):
        n = rs.randint(2, ML + 1)
        base[i, :n] = np.sort(rs.uniform(2.0, 4.8, n)) + rs.uniform(-0.2, 0.2, n)
        base[i, n:2 * n] = np.sort(rs.uniform(0, 80, n))
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
    ap.add_argument("--models", type=int, default=8192)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--base-sites", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bayhunter_amd as bh
    from bayhunter_amd import engine as E
    from bayhunter_amd import datafits as DF
    eng = E.default_engine(0)
    rs = np.random.RandomState(1)
    S, N, NCH = a.sites, a.models, a.chains
    per = np.linspace(2, 60, 30)
    trf = np.arange(201) / 5.0 - 5.0
    sites = []
    for s in range(S):
        t1 = bh.RayleighDispersionPhase(per, 3.4 + 0.01 * per + rs.normal(0, 0.02, per.size))
        t2 = bh.PReceiverFunction(trf, rs.normal(0, 0.02, trf.size))
        t2.moddata.plugin.set_modelparams(gauss=2.5, p=6.4)
        for t in (t1, t2):
            t.set_noise_law("nocorr")
        sites.append(bh.JointTarget([t1, t2]))
    st = bh.SiteTargets(sites)
    m = rows(rs, S * N)
    site = np.repeat(np.arange(S, dtype=np.int32), N)
    vpvs = rs.uniform(1.6, 1.9, S * N).astype(np.float32)
    chain = rs.randint(0, NCH, S * N).astype(np.int32)
    mis = np.abs(rs.normal(0.1, 0.03, S * N)).astype(np.float32)
    kw = dict(engine=eng, max_bytes=1 << 34)
    DF.posterior_datafits(st, m[:4096], vpvs[:4096], site=site[:4096] * 0, chain=chain[:4096], misfits=mis[:4096], **kw)   # warm-up
    r_host, t_host = timed(lambda: DF.posterior_datafits(st, m, vpvs, site=site, chain=chain, misfits=mis, **kw), a.reps)
    md, sd, vd = torch.from_numpy(m).cuda(), torch.from_numpy(site).cuda(), torch.from_numpy(vpvs).cuda()
    cd, fd = torch.from_numpy(chain).cuda(), torch.from_numpy(mis).cuda()
    torch.cuda.synchronize()
    r_dev, t_dev = timed(lambda: DF.posterior_datafits(st, md, vd, site=sd, chain=cd, misfits=fd, **kw), a.reps)
    split = {}
    DF._datafits(st, md, vd, site=sd, chain=cd, misfits=fd, timing=split, **kw)
    agree = all(np.array_equal(r_host[s]["prf"]["quantiles"], r_dev[s]["prf"]["quantiles"], equal_nan=True)
                and np.array_equal(r_host[s]["rdispph"]["median"], r_dev[s]["rdispph"]["median"], equal_nan=True) for s in range(S))

    # the baseline on a few sites, scaled
    nb = min(a.base_sites, S)
    sel = site < nb
    bm, bv, bs = m[sel], vpvs[sel], site[sel]
    t = time.perf_counter()
    nlay, h, vp, vs = bh.Model.pack_batch(bm, bv)
    t_pack = time.perf_counter() - t
    rho = vp * 0.32 + 0.77
    noise = np.tile([0.0, 1.0], (len(bm), 2))
    t = time.perf_counter()
    _, _, err, ymod = st.evaluate_batch(nlay, h, vp, vs, noise, bs, rho=rho, want_ymod=True)
    t_eval = time.perf_counter() - t
    ymod[err != 0] = np.nan
    t = time.perf_counter()
    for s in range(nb):
        np.nanquantile(ymod[bs == s], DF.DEFAULT_QUANTILES, axis=0)
    t_q = time.perf_counter() - t
    scale = S / float(nb)

    # the radix select: R ranks in one call against R calls of one rank
    st._register()
    ld = DF._DataLoaded(md, sd, eng, S)
    try:
        fw = DF._Forward(eng, md.device, DF.DEFAULT_BATCH, ML, 2, eng.ldy)
        fw.fill(ld, DF._per_row(vd, ld.N, "vpvs"), None, None, 0, st._counts())
        cnt = ld.scalar_stats(E.SCALARS_DATA)["count"]
        R = len(DF.DEFAULT_QUANTILES)
        rank = np.zeros(cnt.shape + (R,), np.uint32)
        for r, p in enumerate(DF.DEFAULT_QUANTILES):
            rank[:, :, r] = np.floor((np.maximum(cnt, 1) - 1) * p)
        ld.quantile_keys(E.SCALARS_DATA, rank)
        many, t_many = timed(lambda: ld.quantile_keys(E.SCALARS_DATA, rank), a.reps)
        single, t_single = timed(lambda: [ld.quantile_keys(E.SCALARS_DATA, rank[:, :, r:r + 1]) for r in range(R)], a.reps)
        same_keys = all(np.array_equal(many[0][:, :, r], single[r][0][:, :, 0]) for r in range(R))
    finally:
        ld.close()
    res = dict(sites=S, models_per_site=N, chains=NCH, dtype="float32", layers="2-21", ldy=int(eng.ldy), quantiles=list(DF.DEFAULT_QUANTILES),
               search="engine defaults (short refinement, fast arithmetic)",
               datafits_from_host_rows=t_host, datafits_from_device_rows=t_dev, split_from_device_rows_s=split,
               split_note="one extra run with the device drained after every phase",
               evaluations_per_s_from_device_rows=S * N / t_dev["best_s"],
               host_and_device_agree=bool(agree), failed_rows=int(sum(x["failed"] for x in r_dev)),
               baseline_sites_timed=nb, baseline_pack_batch_s=t_pack, baseline_evaluate_batch_s=t_eval, baseline_np_quantile_s=t_q,
               baseline_all_sites_s_scaled=(t_pack + t_eval + t_q) * scale,
               baseline_note="Model.pack_batch + host evaluate_batch(want_ymod=True) + numpy.nanquantile per site, measured on "
                             "%d sites in this session and SCALED linearly to %d" % (nb, S),
               radix_R=R, radix_multi_rank_call=t_many, radix_R_single_rank_calls=t_single,
               radix_single_over_multi=t_single["best_s"] / t_many["best_s"], radix_same_keys=bool(same_keys))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
