"""Convergence diagnostics of many sites: time of the calls behind DeviceChains.diagnostics (bayhunter_amd.diagnostics.diagnose: the
outlier medians, the sums of likes, vpvs, misfits, noise and of the model series, convergence()) on synthetic AR(1) tables that lie
on the device as record="device" leaves them, best of --reps with the spread.  Beside it, in the same session, the numpy route a
user has today, copy included: the arrays to the host, the vs-at-depth table with numpy, autocovariances with np.fft, the same
convergence().  That route is timed on --numpy-sites of the sites and scaled linearly to all of them (an estimate, and marked so).
Also the counted FP64 multiply-adds of the lag sums of the two largest engine calls over the time between two events of this tool
around each call -- the call's three launches and its copies together: the lag launch alone is not timed here.

    python tools/gpu_chain_diag_perf.py [--sites 64] [--chains 8] [--rows 20000] [--out profiles/chain_diag_perf.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ar1(torch, shape, phi, dev, gen):
    """AR(1) along axis 0, unit innovations, float64 on the device"""
    z = torch.randn(shape, dtype=torch.float64, device=dev, generator=gen)
    x = torch.empty_like(z)
    x[0] = z[0] / np.sqrt(1.0 - phi * phi)
    for t in range(1, shape[0]):
        torch.add(z[t], x[t - 1], alpha=phi, out=x[t])
    return x


def tables(torch, T, Cn, nt, ML, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    f32 = torch.float32
    out = dict(likes=(-1e4 + 3.0 * ar1(torch, (T, Cn), 0.9, dev, gen)).to(f32),
               vpvs=(1.75 + 0.02 * ar1(torch, (T, Cn), 0.8, dev, gen)).to(f32),
               misfits=(0.1 + 0.01 * ar1(torch, (T, Cn, nt + 1), 0.9, dev, gen)).abs().to(f32),
               noise=(0.05 + 0.003 * ar1(torch, (T, Cn, 2 * nt), 0.95, dev, gen)).to(f32))
    out["noise"][:, :, 0::2] = 0.0                                  # fixed correlations
    n = 2 + torch.arange(Cn, device=dev) % (ML - 1)                 # layers per chain: 2..ML
    j = torch.arange(ML, device=dev)
    on = (j[None, :] < n[:, None])                                  # [C][ML]
    vs = 2.5 + 0.1 * j[None, None, :] + 0.05 * ar1(torch, (T, Cn, ML), 0.9, dev, gen)
    z = 80.0 * (j[None, None, :] + 0.5) / n[None, :, None] + 0.2 * ar1(torch, (T, Cn, ML), 0.9, dev, gen).clamp(-4, 4)
    z = torch.sort(torch.where(on[None], z, torch.full_like(z, 1e9)), dim=2).values
    nan = torch.full_like(vs, float("nan"))
    models = torch.full((T, Cn, 2 * ML), float("nan"), dtype=f32, device=dev)
    both = torch.cat((torch.where(on[None], vs, nan), torch.where(on[None], z, nan)), dim=2)    # [T][C][2ML]: vs.., NaN.., z.., NaN..
    # the reference's row: the n vs, then the n depths, then NaN
    pos = torch.arange(2 * ML, device=dev)[None, :]
    src = torch.where(pos < n[:, None], pos, ML + (pos - n[:, None])).clamp(0, 2 * ML - 1)       # [C][2ML]
    row = torch.gather(both, 2, src[None].expand(T, Cn, 2 * ML))
    models[:] = torch.where(pos[None] < 2 * n[None, :, None], row, torch.full_like(row, float("nan"))).to(f32)
    out["models"] = models
    return out


def vs_table(models, dep, chunk=100000):
    """numpy: vs at dep and nlayers of rows [N][2ML] (the rule of posterior_models), chunked"""
    N, W = models.shape
    ML = W // 2
    out = np.empty((N, dep.size + 1))
    for r0 in range(0, N, chunk):
        m = models[r0:r0 + chunk]
        n = (~np.isnan(m)).sum(axis=1) // 2
        j = np.arange(ML)
        vs = np.take_along_axis(m, np.minimum(j[None, :], n[:, None] - 1), axis=1)
        z = np.take_along_axis(m, np.minimum(n[:, None] + j[None, :], 2 * n[:, None] - 1), axis=1)
        zd = (z[:, :-1] + z[:, 1:]) / np.float32(2)
        h = np.diff(np.concatenate((np.zeros((len(m), 1)), zd.astype(np.float64)), axis=1), axis=1)
        d = np.cumsum(h, axis=1)
        d[j[None, :-1] >= n[:, None] - 1] = np.inf
        k = np.zeros((len(m), dep.size), np.int64)
        for jj in range(ML - 1):
            k += d[:, jj:jj + 1] <= dep[None, :]
        out[r0:r0 + chunk, :-1] = np.take_along_axis(vs, k, axis=1)
        out[r0:r0 + chunk, -1] = n - 1
    return out


def numpy_tables(x, L):
    """the table of chain_series_stats with numpy: sums directly, lag sums by FFT"""
    x = np.asarray(x, np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    T = x.shape[0]
    h = T // 2
    x0 = x[0]
    d = x - x0
    s1, s1a, s1b = d.sum(axis=0), d[:h].sum(axis=0), d[T - h:].sum(axis=0)
    e = d - s1 / T
    F = np.fft.rfft(e, n=2 * T, axis=0)
    p = np.fft.irfft(F * np.conj(F), n=2 * T, axis=0)[:L + 1]
    return dict(x0=x0, s1=s1, s1a=s1a, s1b=s1b, m2a=((d[:h] - s1a / h) ** 2).sum(axis=0), m2b=((d[T - h:] - s1b / h) ** 2).sum(axis=0),
                p=np.ascontiguousarray(np.moveaxis(p, 0, -1)), T=T, maxlag=L)


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
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--nt", type=int, default=3)
    ap.add_argument("--depths", type=int, default=41)
    ap.add_argument("--maxlag", type=int, default=1000)
    ap.add_argument("--layers", type=int, default=21)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--numpy-sites", type=int, default=2)
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
    tabs = tables(torch, T, Cn, a.nt, a.layers, dev)
    torch.cuda.synchronize()
    site_of, ids = np.arange(Cn) // Cs, np.arange(Cn)
    small = {k: v[:64, :Cs] for k, v in tabs.items()}
    D.diagnose(small, site_of[:Cs], ids[:Cs], dep=dep, maxlag=8, engine=eng)          # warm-up (code objects, allocations)
    r_dev, t_dev = timed(lambda: D.diagnose(tabs, site_of, ids, dep=dep, maxlag=L, engine=eng), a.reps)

    def events(fn):
        times = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3)
        return dict(best_s=min(times), all_s=times, spread_s=max(times) - min(times))

    macs_per_series = sum(max(0, T - k) for k in range(L + 1))
    ev_models = events(lambda: D.chain_model_stats(tabs["models"], dep, L, engine=eng))
    ev_noise = events(lambda: D.chain_series_stats(tabs["noise"], L, engine=eng))
    ev_models0 = events(lambda: D.chain_model_stats(tabs["models"], dep, 0, engine=eng))
    macs_models, macs_noise = macs_per_series * Cn * (a.depths + 1), macs_per_series * Cn * 2 * a.nt

    # the numpy route on the first sites, scaled to all of them
    Sn = min(a.numpy_sites, S)
    cn = Sn * Cs

    def numpy_route():
        host = {k: v[:, :cn].cpu().numpy() for k, v in tabs.items()}
        outl, _ = D.outlier_chains(host["likes"], site_of[:cn])
        ex = np.concatenate(outl)
        res = {k: D.convergence(numpy_tables(host[k], L), site_of[:cn], ex) for k in ("likes", "vpvs", "misfits", "noise")}
        vt = vs_table(host["models"].reshape(T * cn, -1), dep).reshape(T, cn, -1)
        res["vs"] = D.convergence(numpy_tables(vt, L), site_of[:cn], ex)
        return res
    r_np, t_np = timed(numpy_route, 1)
    rh_dev, rh_np = r_dev[0]["vs"]["rhat"], r_np["vs"][0]["rhat"][:a.depths]
    ess_dev, ess_np = r_dev[0]["misfits"]["ess"], r_np["misfits"][0]["ess"]
    scale = float(S) / Sn
    res = dict(sites=S, chains_per_site=Cs, rows=T, nt=a.nt, depths=a.depths, maxlag=L, layers_max=a.layers, dtype="float32",
               series=Cn * (2 + a.nt + 1 + 2 * a.nt + a.depths + 1),
               device_route=t_dev, device_route_note="diagnose() on device tensors: medians, 5 engine calls, the copies of the sums to the "
                                                     "host, convergence() in numpy",
               numpy_route_sites_timed=Sn, numpy_route_timed=t_np, numpy_route_s_all_sites_est=t_np["best_s"] * scale,
               numpy_route_note="device->host copy, vs table with numpy, np.fft autocovariances, convergence(); timed once on %d of %d "
                                "sites and scaled linearly: an estimate" % (Sn, S),
               device_faster=bool(t_dev["best_s"] < t_np["best_s"] * scale),
               models_call_events=ev_models, models_call_maxlag0_events=ev_models0, noise_call_events=ev_noise,
               lag_multiply_adds_models_call=macs_models, lag_multiply_adds_noise_call=macs_noise,
               multiply_adds_per_s_models_call=macs_models / ev_models["best_s"], multiply_adds_per_s_noise_call=macs_noise / ev_noise["best_s"],
               rate_note="counted multiply-adds sum_k (T - k) per series over the time of the WHOLE engine call between two events of "
                         "this tool (three launches, the copy of the lag sums to the host): a lower bound of the lag launch's rate; "
                         "the lag launch alone, and every other kernel alone, is unmeasured",
               agreement=dict(vs_rhat_max_rel=float(np.nanmax(np.abs(rh_dev - rh_np) / np.abs(rh_np))),
                              misfits_ess_max_rel=float(np.nanmax(np.abs(ess_dev - ess_np) / np.abs(ess_np)))))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
