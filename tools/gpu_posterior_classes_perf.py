"""Conditional posteriors of many sites: time of one posterior_classes call on S sites x N float32 models on the device (A), and
of its class-forming stage alone (bh_posterior_classes on a handle whose sets are formed), best of --reps with the spread.  Beside
it the route a user has without that call and without a host copy (B): the same columns -- the Moho depth and a velocity drop --
formed with torch operations on the padded [N, ML] tables of the rows as tools/gpu_posterior_features_perf.py forms them, then
torch comparisons and a bincount for cls and counts; its class-forming stage (the comparisons and the bincount, the columns
given) alone likewise.  Four classes: the Moho in the upper or the lower half of the site's range, crossed with a drop present or
absent; a row without a Moho is in no class.

B is written to give A's bits, and the tool asserts it: cls of every row and counts of every (site, class).

The bar: A's class-forming stage no slower than B's by more than the spread of B's repeats.

Also reported, without a bar: posterior_models(classes=) against posterior_models on the same rows -- the cost of four times as
many sites.

    python tools/gpu_posterior_classes_perf.py [--sites 64] [--models 200000] [--out profiles/posterior_classes_perf.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.gpu_posterior_moho_perf import rows, timed   # noqa: E402
from tools.gpu_posterior_features_perf import torch_features   # noqa: E402

MOHOVS = 4.0
NAMES = ("upper_lvz", "upper", "lower_lvz", "lower")


def site_rule(rs, S):
    """every site's Moho range (lo, hi) and drop threshold; the rule over them; B's features: `above` with the Moho's parameters
    is the Moho set's depth bit for bit (include/bh_engine_posterior_features.h)"""
    lo, hi, c = 15.0 * rs.uniform(0.9, 1.1, S), 55.0 * rs.uniform(0.9, 1.1, S), 0.3 * rs.uniform(0.9, 1.1, S)
    mid = (lo + hi) / 2
    classes = {"upper_lvz": [("moho", lo, mid), ("lvz.depth", "has")], "upper": [("moho", lo, mid)],
               "lower_lvz": [("moho", mid, hi), ("lvz.depth", "has")], "lower": [("moho", mid, hi)]}
    feats_a = dict(lvz=("drop", 5.0, 60.0, c))
    feats_b = dict(moho=("above", lo, hi, np.full(S, MOHOVS)), lvz=("drop", 5.0, 60.0, c))
    return lo, mid, hi, classes, feats_a, feats_b


def torch_classes(torch, moho, drop, site, lo, mid, hi, S):
    """B's class-forming stage: (cls int32 [N], counts int64 [S, 5]) from the columns with torch comparisons"""
    up = (moho >= lo[site]) & (moho < mid[site])          # (a NaN compares false: a row without a Moho is in no class)
    low = (moho >= mid[site]) & (moho < hi[site])
    has = ~torch.isnan(drop)
    none = torch.full_like(site, -1)
    cls = torch.where(up & has, 0, torch.where(up, 1, torch.where(low & has, 2, torch.where(low, 3, none))))
    counts = torch.bincount(site * 5 + torch.where(cls < 0, 4, cls), minlength=S * 5).reshape(S, 5)
    return cls.to(torch.int32), counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=64)
    ap.add_argument("--models", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from bayhunter_amd import engine as E
    from bayhunter_amd.posterior import _Loaded, check_classes, check_features, posterior_classes, posterior_models
    eng = E.Engine(0)
    rs = np.random.RandomState(1)
    S, N = a.sites, a.models
    m = rows(rs, S * N)
    site = np.repeat(np.arange(S, dtype=np.int32), N)
    lo, mid, hi, classes, feats_a, feats_b = site_rule(rs, S)
    moho = np.stack((lo, hi), axis=1)
    md, sd = torch.from_numpy(m).cuda(), torch.from_numpy(site).cuda()
    sl = sd.long()
    del m
    kinds_a, par_a, labels_a = check_features(feats_a, S)
    kinds_b, par_b, labels_b = check_features(feats_b, S)
    assert labels_b == ["moho", "lvz.depth", "lvz.jump"]
    pard = torch.from_numpy(par_b).cuda()
    lod, midd, hid = (torch.from_numpy(v).cuda() for v in (lo, mid, hi))
    labels = {"moho": (E.SCALARS_MOHO, 0), "lvz.depth": (E.SCALARS_FEATURES, 0), "lvz.jump": (E.SCALARS_FEATURES, 1)}
    names, tc, ts, tq, to, tlo, thi = check_classes(classes, S, labels)
    assert tuple(names) == NAMES

    def whole_a():
        return posterior_classes(md, classes, site=sd, features=feats_a, moho=moho, mohovs=MOHOVS, engine=eng, nsites=S)

    def columns_b():
        cols = torch_features(torch, md, sl, kinds_b, pard)
        torch.cuda.synchronize()
        return cols

    def whole_b():
        cols = torch_features(torch, md, sl, kinds_b, pard)
        out = torch_classes(torch, cols[0], cols[1], sl, lod, midd, hid, S)
        counts = out[1].cpu()                                                   # (the counts on the host, as A returns them)
        return out[0], counts

    w = slice(0, 4096)                                                          # warm-up (code objects, allocations)
    posterior_classes(md[w], classes, site=sd[w], features=feats_a, moho=moho, mohovs=MOHOVS, engine=eng, nsites=S)
    cw = torch_features(torch, md[w], sl[w], kinds_b, pard)
    torch_classes(torch, cw[0], cw[1], sl[w], lod, midd, hid, S)
    posterior_models(md[w], site=sd[w], engine=eng, nsites=S)
    torch.cuda.synchronize()

    ld = _Loaded(md, sd, eng, S, scalars=True)
    try:
        ld.features(kinds_a, par_a)
        ld.moho(lo, hi, np.full(S, MOHOVS))
        (cls_a, cnt_a), t_form_a = timed(lambda: ld.classes(4, tc, ts, tq, to, tlo, thi, device=md.device), a.reps)
    finally:
        ld.close()
    cols_b, t_cols_b = timed(columns_b, a.reps)

    def form_b():
        out = torch_classes(torch, cols_b[0], cols_b[1], sl, lod, midd, hid, S)
        counts = out[1].cpu()
        return out[0], counts

    (cls_b, cnt_b), t_form_b = timed(form_b, a.reps)
    assert torch.equal(cls_a, cls_b), "B's classes are not A's"
    assert np.array_equal(cnt_a, cnt_b.numpy()), "B's counts are not A's"
    assert (cnt_a.sum(1) == N).all() and (cnt_a.sum(0) > 0).all()               # every class and "no class" hold rows
    del cols_b, cls_b
    r_a, t_a = timed(whole_a, a.reps)
    r_b, t_b = timed(whole_b, a.reps)
    assert torch.equal(r_a["cls"], r_b[0]) and np.array_equal(r_a["counts"], r_b[1].numpy()[:, :4])
    # the cost of four times as many sites: posterior_models over the classes against posterior_models over the sites
    pm_c, t_models_classes = timed(lambda: posterior_models(md, site=sd, engine=eng, nsites=S, classes=r_a), a.reps)
    pm, t_models = timed(lambda: posterior_models(md, site=sd, engine=eng, nsites=S), a.reps)
    assert sum(pm_c[0][k]["count"] for k in NAMES) == N - int(r_a["unclassified"][0]) and pm[0]["count"] == N
    met = t_form_a["best_s"] <= t_form_b["best_s"] + t_form_b["spread_s"]
    res = dict(sites=S, models_per_site=N, dtype="float32", layers="2-21", classes=list(NAMES), terms=int(tc.size),
               rows_per_class_site0={k: int(v) for k, v in zip(NAMES + ("none",), cnt_a[0])},
               A_posterior_classes_from_device_rows=t_a, A_class_forming_call=t_form_a,
               B_torch_columns_and_comparisons=t_b, B_torch_columns_alone=t_cols_b, B_class_forming_torch_comparisons=t_form_b,
               bar="A's class-forming stage no slower than B's by more than the spread of B's repeats",
               bar_met=bool(met), forming_ratio_B_over_A=t_form_b["best_s"] / t_form_a["best_s"],
               whole_speedup_A_over_B=t_b["best_s"] / t_a["best_s"], same_bits=True,
               posterior_models_over_classes=t_models_classes, posterior_models_over_sites=t_models,
               models_classes_over_sites=t_models_classes["best_s"] / t_models["best_s"],
               per_kernel_times="in profiles/posterior_classes_kernels.txt: one rocprofv3 --kernel-trace --stats run of this workload")
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
