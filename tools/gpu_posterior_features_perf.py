"""Structural features of many sites: time of one posterior_features call on S sites x N float32 models on the device (A), and of
its feature-forming call alone (bh_posterior_features), best of --reps with the spread.  Beside it the route a user has without
that call and without a host copy (B): the same columns formed with torch operations on the padded [N, ML] tables of the rows,
then posterior_scalars(columns=...) on them; its feature-forming stage alone likewise.

B is written to give A's bits, and the tool asserts it (on --check-rows rows picked at random, and on the exact statistics of
every whole column): a row's float64 sums run over its layers in ascending order, so B walks the ML layers in a Python loop of
elementwise operations on [N] vectors -- torch.cumsum and the index of torch.min promise neither the order of the additions nor the
first of equal values.

The bar: A's feature-forming stage no slower than B's by more than the spread of B's repeats.

    python tools/gpu_posterior_features_perf.py [--sites 64] [--models 200000] [--out profiles/posterior_features_perf.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.gpu_posterior_moho_perf import rows, timed   # noqa: E402

# eight features, one of every row of the table of kinds (vsmin stands for vsmax, the same walk with the other comparison)
FEATURES = dict(upper=("vsmean", 0.0, 15.0), vs1k=("vstime", 0.0, 1.0), sed_t=("tts", 0.0, 3.0), slow=("vsmin", 5.0, 60.0),
                lvz=("drop", 5.0, 60.0, 0.3), step=("jump", 10.0, 55.0, 0.5), basement=("above", 0.0, 20.0, 3.2),
                crustal=("nifaces", 0.0, 40.0))


def site_features(rs, S):
    """FEATURES with every site's own window ends and thresholds"""
    out = {}
    for name, f in FEATURES.items():
        z1 = f[2] * rs.uniform(0.9, 1.1, S)
        out[name] = (f[0], f[1], z1) + ((f[3] * rs.uniform(0.9, 1.1, S),) if len(f) == 4 else ())
    return out


def torch_features(torch, models, site, kinds, par):
    """B's feature-forming stage: {label index: float64 [N] device tensor} of the columns of bh_posterior_features, from the rows
    [N, 2 ML] (float32, device), site [N] (int64) and the table par [S, F, 3] (device), with torch operations only."""
    from bayhunter_amd.posterior import FEATURE_KINDS
    N, W = models.shape
    ML = W // 2
    f64, inf, nan = torch.float64, float("inf"), float("nan")
    n = (~torch.isnan(models)).sum(1) // 2
    colsi = torch.arange(ML, device=models.device)
    z = torch.gather(models, 1, torch.clamp(n[:, None] + colsi[None, :], max=W - 1)).t().contiguous()
    vs = models[:, :ML].t().contiguous()                              # [ML, N]: a layer of all rows lies together
    zd = (z[:-1] + z[1:]) / 2                                         # float32; NaN or foreign from n - 1 on, never used there
    d, acc, prev = [], None, torch.zeros(N, dtype=f64, device=models.device)
    for j in range(ML - 1):
        zj = zd[j].to(f64)
        h = zj - prev
        acc = h if j == 0 else acc + h
        d.append(acc)
        prev = zj
    zero = torch.zeros(N, dtype=f64, device=models.device)
    fnan = torch.full((N,), nan, dtype=f64, device=models.device)
    finf = torch.full((N,), inf, dtype=f64, device=models.device)

    def fin(x):
        return torch.where(torch.isfinite(x), x, fnan)

    out = []
    for f, k in enumerate(kinds):
        kind = FEATURE_KINDS[k]
        p = par[site, f]
        z0, z1, c = p[:, 0].contiguous(), p[:, 1].contiguous(), p[:, 2].contiguous()
        if kind in ("vsmean", "vstime", "tts", "vsmin", "vsmax"):
            s, t = zero, zero
            have = torch.zeros(N, dtype=torch.bool, device=models.device)
            a, b = fnan, fnan
            for j in range(ML):
                bj = torch.where(j < n - 1, d[j], finf) if j < ML - 1 else finf
                top = torch.maximum(t, z0)
                ln = torch.minimum(bj, z1) - top
                inw = (j < n) & (ln > 0)
                v = vs[j].to(f64)
                if kind in ("vsmin", "vsmax"):
                    better = inw & (~have | ((v > a) if kind == "vsmax" else (v < a)))
                    a, b = torch.where(better, v, a), torch.where(better, top, b)
                    have = have | inw
                else:
                    s = s + torch.where(inw, v * ln if kind == "vsmean" else ln / v, zero)
                t = bj
            if kind in ("vsmin", "vsmax"):
                out += [fin(a), fin(b)]
            else:
                out.append(fin(s / (z1 - z0) if kind == "vsmean" else (z1 - z0) / s if kind == "vstime" else s))
            continue
        have = torch.zeros(N, dtype=torch.bool, device=models.device)
        best, dep, cnt = zero, zero, zero
        for k2 in range(ML - 1):
            inw = (k2 < n - 1) & (d[k2] > z0) & (d[k2] < z1)
            if kind == "nifaces":
                cnt = cnt + inw.to(f64)
                continue
            if kind == "above":
                better = inw & ~have & (vs[k2 + 1].to(f64) > c)
                dep = torch.where(better, d[k2], dep)
                have = have | better
                continue
            jm = (vs[k2 + 1] - vs[k2]).to(f64)         # the row dtype's subtraction
            better = inw & (~have | ((jm > best) if kind == "jump" else (jm < best)))
            best, dep = torch.where(better, jm, best), torch.where(better, d[k2], dep)
            have = have | inw
        if kind == "nifaces":
            out.append(cnt)
        elif kind == "above":
            out.append(fin(torch.where(have, dep, fnan)))
        else:
            on = have & ((best > c) if kind == "jump" else (best < -c))
            out += [fin(torch.where(on, dep, fnan)), fin(torch.where(on, best, fnan))]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=64)
    ap.add_argument("--models", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--check-rows", type=int, default=1000000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from bayhunter_amd import engine as E
    from bayhunter_amd.posterior import _Loaded, check_features, posterior_features, posterior_scalars
    eng = E.Engine(0)
    rs = np.random.RandomState(1)
    S, N = a.sites, a.models
    m = rows(rs, S * N)
    site = np.repeat(np.arange(S, dtype=np.int32), N)
    feats = site_features(rs, S)
    kinds, par, labels = check_features(feats, S)
    md, sd = torch.from_numpy(m).cuda(), torch.from_numpy(site).cuda()
    sl, pard = sd.long(), torch.from_numpy(par).cuda()
    del m

    def form_b():
        cols = torch_features(torch, md, sl, kinds, pard)
        torch.cuda.synchronize()
        return cols

    def whole_b():
        cols = form_b()
        return posterior_scalars(md, dict(zip(labels, cols)), site=sd, bins=50, nlayers=False, engine=eng, nsites=S)

    w = slice(0, 4096)                                                          # warm-up (code objects, allocations)
    posterior_features(md[w], FEATURES, engine=eng)
    posterior_scalars(md[w], dict(zip(labels, torch_features(torch, md[w], sl[w] * 0, kinds, pard))), nlayers=False, engine=eng)
    ld = _Loaded(md, sd, eng, S, scalars=True)
    try:
        found, t_form_a = timed(lambda: ld.features(kinds, par), a.reps)
        cols_b, t_form_b = timed(form_b, a.reps)
        # the same bits: rows picked at random through their input index, then the exact statistics of the whole columns
        st_a = ld.scalar_stats(E.SCALARS_FEATURES)
        ld.attach(torch.arange(S * N, dtype=torch.float64, device=md.device)[:, None], False)
        pos = np.sort(rs.choice(S * N, min(a.check_rows, S * N), replace=False))
        orig = torch.from_numpy(ld.gather(E.SCALARS_USER, pos, 1)[:, 0].astype(np.int64)).cuda()
        ta = ld.gather(E.SCALARS_FEATURES, pos, len(labels))
        tb = torch.stack([c[orig] for c in cols_b], dim=1).cpu().numpy()
        assert np.array_equal(ta, tb, equal_nan=True), "B's columns are not A's bits"
        ld.attach(torch.stack(cols_b, dim=1), False)
        st_b = ld.scalar_stats(E.SCALARS_USER)
        for key in ("count", "nan", "kmin", "kmax", "scale", "x0", "sums", "median"):
            assert np.array_equal(st_a[key], st_b[key]), "B's column statistics are not A's: " + key
        assert np.array_equal(found, st_a["count"])
    finally:
        ld.close()
    del cols_b
    r_a, t_a = timed(lambda: posterior_features(md, feats, site=sd, engine=eng, nsites=S), a.reps)
    r_b, t_b = timed(whole_b, a.reps)
    for s in (0, S - 1):
        for q, name in enumerate(labels):
            da = r_a[s][name.split(".")[0]]
            da = da[name.split(".")[1]] if "." in name else da
            for key in ("count", "median", "min", "max", "mean", "std"):
                assert da[key] == r_b[s][name][key] or (da[key] != da[key] and r_b[s][name][key] != r_b[s][name][key]), (s, name, key)
    met = t_form_a["best_s"] <= t_form_b["best_s"] + t_form_b["spread_s"]
    res = dict(sites=S, models_per_site=N, dtype="float32", layers="2-21", bins=50, features=len(feats), columns=len(labels),
               kinds=[f[0] for f in feats.values()],
               A_posterior_features_from_device_rows=t_a, A_feature_forming_call=t_form_a,
               B_torch_columns_then_posterior_scalars=t_b, B_feature_forming_torch_ops=t_form_b,
               bar="A's feature-forming stage no slower than B's by more than the spread of B's repeats",
               bar_met=bool(met), forming_speedup_A_over_B=t_form_b["best_s"] / t_form_a["best_s"],
               whole_speedup_A_over_B=t_b["best_s"] / t_a["best_s"],
               same_bits_checked_rows=int(len(pos)), same_bits=True,
               probability_site0={k: r_a[0][k]["probability"] for k in ("lvz", "step", "basement")},
               per_kernel_times="in profiles/posterior_features_kernels.txt: one rocprofv3 --kernel-trace --stats run of this workload")
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
