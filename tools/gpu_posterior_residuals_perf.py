"""Posterior residuals of many sites: time of one posterior_residuals call (maxlag 10, the default five quantiles) on S sites x N
float32 rows, Rayleigh phase at 30 periods + a P receiver function of 201 samples, prior-like rows of 2-21 layers (the workload
of tools/gpu_posterior_datafits_perf.py), with the engine's default search and arithmetic, from device rows.

(A) posterior_residuals: the whole call, best of --reps with the spread, and its residual-forming stage alone -- the "residuals"
    lap of the forward loop (bh_posterior_resid_fill), the device drained after every lap.
(B) the route without the kernel and without a host copy: the same forward loop with the columns formed per batch by torch
    operations on the ymod tensor (slices, products, sums), then posterior_scalars(columns=).  Its column-forming stage is timed the
    same way.  The largest |A - B| over all columns of all rows is recorded (the same numbers to rounding, not the same bits).
The bar: A's stage is no slower than B's by more than the spread of B's repeats -- reported met or missed as measured.
Also: the fill's share against the forward lap, and posterior_datafits(residuals=) against the two calls made separately.

    python tools/gpu_posterior_residuals_perf.py [--sites 64] [--models 100000] [--out profiles/posterior_residuals_perf.json]
    --only-a: (A) once and nothing else (the run under rocprofv3 --kernel-trace --stats)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gpu_posterior_datafits_perf import ML, rows, timed   # noqa: E402


def stat(times):
    return dict(best_s=min(times), all_s=list(times), spread_s=max(times) - min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=64)
    ap.add_argument("--models", type=int, default=100000)
    ap.add_argument("--maxlag", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only-a", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bayhunter_amd as bh
    from bayhunter_amd import engine as E
    from bayhunter_amd import datafits as DF
    eng = E.default_engine(0)
    rs = np.random.RandomState(1)
    S, N, L = a.sites, a.models, a.maxlag
    per = np.linspace(2, 60, 30)
    trf = np.arange(201) / 5.0 - 5.0
    sites = []
    for s in range(S):
        t1 = bh.RayleighDispersionPhase(per, 3.4 + 0.01 * per + rs.normal(0, 0.02, per.size))
        t2 = bh.PReceiverFunction(trf, rs.normal(0, 0.02, trf.size))
        t2.moddata.plugin.set_modelparams(gauss=2.5, p=6.4)
        t1.set_noise_law("nocorr")
        t2.set_noise_law("exp")
        sites.append(bh.JointTarget([t1, t2]))
    st = bh.SiteTargets(sites)
    m = rows(rs, S * N)
    site = np.repeat(np.arange(S, dtype=np.int32), N)
    vpvs = rs.uniform(1.6, 1.9, S * N).astype(np.float32)
    noise = np.stack([np.zeros(S * N), rs.uniform(0.01, 0.05, S * N), rs.uniform(0.5, 0.99, S * N), rs.uniform(0.005, 0.03, S * N)],
                     axis=1).astype(np.float32)
    kw = dict(engine=eng, max_bytes=1 << 34)
    md, sd, vd, nd = (torch.from_numpy(x).cuda() for x in (m, site, vpvs, noise))
    dev = md.device
    torch.cuda.synchronize()
    call_a = lambda: DF.posterior_residuals(st, md, vd, nd, site=sd, maxlag=L, **kw)
    DF.posterior_residuals(st, md[:4096], vd[:4096], nd[:4096], site=sd[:4096] * 0, maxlag=L, **kw)   # warm-up
    if a.only_a:
        call_a()
        torch.cuda.synchronize()
        return
    r_a, t_a = timed(call_a, a.reps)
    splits = []
    for _ in range(a.reps):
        sp = {}
        DF._datafits(st, md, vd, site=sd, timing=sp, data=False, residuals=dict(noise=nd, maxlag=L), **kw)
        splits.append(sp)
    a_stage = stat([sp["residuals"] for sp in splits])
    a_forward = stat([sp["forward"] for sp in splits])

    # (B) the torch route on the same forward loop
    st._register()
    ncol = st._counts()
    off = np.concatenate(([0], np.cumsum(ncol.max(axis=0)))).astype(int)
    yobs, g, _ = DF._resid_tables(st)
    yobs_d = torch.from_numpy(yobs).cuda()
    nt, W = st.ntargets, E.RESID_FIXED + L
    nan = float("nan")

    def torch_columns(ym, err, s, nz):
        """[nb, nt * W]: the header's columns by torch operations on the batch's synthetics"""
        e = ym - yobs_d[s]
        cols = []
        for t in range(nt):
            n = int(ncol[0, t])
            u = e[:, off[t]:off[t] + n]
            corr, sigma = nz[:, 2 * t].double(), nz[:, 2 * t + 1].double()
            a0 = (u * u).sum(1)
            acf = [(u[:, :n - l] * u[:, l:]).sum(1) / a0 for l in range(1, L + 1)]
            cols += [u.sum(1) / n, torch.sqrt(a0 / n), torch.sqrt(a0 / n) / sigma, corr, acf[0] - corr] + acf
        out = torch.stack(cols, dim=1)
        return torch.where((err != 0)[:, None], torch.full_like(out, nan), out)

    ld = DF._DataLoaded(md, sd, eng, S)
    try:
        ld.attach(torch.arange(ld.N, dtype=torch.float64, device=dev)[:, None], False)
        orig = torch.from_numpy(ld.gather(E.SCALARS_USER, np.arange(ld.nrows), 1)[:, 0].astype(np.int64)).cuda()
        fw = DF._Forward(eng, dev, DF.DEFAULT_BATCH, ML, nt, eng.ldy)
        vt = DF._per_row(vd, ld.N, "vpvs")
        buf = fw.buf
        ptr = lambda k: C.c_void_p(buf[k].data_ptr())
        b_loaded = torch.empty((ld.nrows, nt * W), dtype=torch.float64, device=dev)
        b_stage_t, b_forward_t, b_total_t = [], [], []
        for _ in range(a.reps + 1):                                           # (the first pass warms the torch kernels up)
            torch.cuda.synchronize()
            t_stage = t_fwd = 0.0
            t0 = time.perf_counter()
            for r0, r1 in DF.plan_batches(ld.nrows, fw.B):
                nb = r1 - r0
                t1 = time.perf_counter()
                ld.layers(r0, r1, vt, None, None, buf, fw.B)
                eng.evaluate_sites_dev(nb, ML, ptr("nlay"), ptr("h"), ptr("vp"), ptr("vs"), ptr("rho"), fw.B, 1, ptr("site"), ptr("noise"),
                                       ptr("logL"), ptr("misf"), ptr("err"), ymod=ptr("ymod"), stream=fw.stream)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                b_loaded[r0:r1] = torch_columns(buf["ymod"][:nb], buf["err"][:nb], buf["site"][:nb].long(), nd[orig[r0:r1]])
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                t_fwd += t2 - t1
                t_stage += t3 - t2
            b_input = torch.empty_like(b_loaded)
            b_input[orig] = b_loaded
            r_b = bh.posterior_scalars(md, dict(c=b_input), site=sd, nlayers=False, engine=eng, nsites=S, quantiles=DF.DEFAULT_QUANTILES)
            torch.cuda.synchronize()
            b_total_t.append(time.perf_counter() - t0)
            b_stage_t.append(t_stage)
            b_forward_t.append(t_fwd)
        b_stage, b_forward, b_total = stat(b_stage_t[1:]), stat(b_forward_t[1:]), stat(b_total_t[1:])
        # the largest |A - B| over the columns of all rows: A's set by input row against B's
        fw.fill(ld, vt, None, None, 0, ncol, data=False, resid=dict(L=L, yobs=yobs, g=g, noise=DF._noise_rows(nd, ld.N, nt)))
        a_input = ld.export(E.SCALARS_RESID, device=dev)
        both_nan = torch.isnan(a_input) & torch.isnan(b_input)
        nan_differs = int((torch.isnan(a_input) != torch.isnan(b_input)).sum().item())
        diff = torch.where(both_nan, torch.zeros_like(a_input), (a_input - b_input).abs())
        max_abs = float(torch.nan_to_num(diff, nan=0.0).max().item())
        med_diff = max(abs(r_a[s]["prf"]["acf"]["median"][l] - r_b[s]["c"][W + E.RESID_FIXED + l]["median"]) for s in range(S) for l in range(L))
    finally:
        ld.close()

    # one forward pass for both sets against the two calls made separately
    call_both = lambda: DF.posterior_datafits(st, md, vd, site=sd, residuals=dict(noise=nd, maxlag=L), **kw)
    call_two = lambda: (DF.posterior_datafits(st, md, vd, site=sd, **kw), call_a())
    call_both()
    _, t_both = timed(call_both, a.reps)
    _, t_two = timed(call_two, a.reps)

    met = a_stage["best_s"] <= b_stage["best_s"] + b_stage["spread_s"]
    res = dict(sites=S, models_per_site=N, dtype="float32", layers="2-21", ldy=int(eng.ldy), maxlag=L, resid_columns=nt * W,
               quantiles=list(DF.DEFAULT_QUANTILES), search="engine defaults (short refinement, fast arithmetic)",
               A_posterior_residuals_call=t_a, A_split_s=splits,
               split_note="%d extra runs with the device drained after every phase" % a.reps,
               A_residual_stage=a_stage, A_forward_lap=a_forward, A_stage_over_forward=a_stage["best_s"] / a_forward["best_s"],
               A_stage_share_of_call=a_stage["best_s"] / t_a["best_s"],
               B_torch_route_total=b_total, B_column_stage=b_stage, B_forward_lap=b_forward,
               B_note="the forward loop with the columns formed per batch by torch operations on ymod (drained after the forward "
                      "launch and after the columns), then posterior_scalars(columns=); one untimed warm-up pass",
               max_abs_A_minus_B_over_all_columns=max_abs, nan_masks_differ_in=nan_differs, max_abs_median_acf_A_minus_B=float(med_diff),
               bar="A's residual-forming stage no slower than B's by more than the spread of B's repeats",
               bar_result="met" if met else "missed", B_stage_over_A_stage=b_stage["best_s"] / a_stage["best_s"],
               datafits_with_residuals_one_pass=t_both, datafits_and_residuals_two_calls=t_two,
               two_calls_over_one_pass=t_two["best_s"] / t_both["best_s"], failed_rows=int(sum(x["failed"] for x in r_a)))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
