"""Convergence of structural features of many sites: time of the feature series of the chains (A: diagnostics.chain_feature_series,
one engine call on the store's model rows where they lie) and of the whole DeviceChains.diagnostics(features=) behind it
(diagnostics.diagnose), on the workload of tools/gpu_chain_diag_perf.py -- S sites x 8 chains x T float32 rows on the device -- with
the eight features of tools/gpu_posterior_features_perf.py (11 columns, every site its own windows and thresholds).  Best of --reps
with the spread, in one session.

Beside it the route a user has without that call and without a host copy (B): posterior_classes(return_columns=True) on the same
rows -- the load scatters them by site, bh_posterior_features forms the columns, the export brings them back by input row --, the
columns reshaped to [T][C], stacked, and the NaNs replaced with torch; then the same downstream call (feature_convergence).  The
two routes must give the same value / present bits: asserted here on the whole tables.

The bar: A's column-forming stage no slower than B's by more than the spread of B's repeats.

    python tools/gpu_chain_diag_features_perf.py [--sites 64] [--chains 8] [--rows 20000] [--out profiles/chain_diag_features_perf.json]
    --trace: the two column-forming stages alone, twice each (the first pass is the warm-up), for rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.gpu_chain_diag_perf import tables, timed                  # noqa: E402
from tools.gpu_posterior_features_perf import site_features          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=64)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--nt", type=int, default=3)
    ap.add_argument("--maxlag", type=int, default=1000)
    ap.add_argument("--layers", type=int, default=21)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from bayhunter_amd import diagnostics as D
    from bayhunter_amd import engine as E
    from bayhunter_amd.posterior import posterior_classes
    eng = E.default_engine(0)
    dev = torch.device("cuda", 0)
    S, Cs, T, L = a.sites, a.chains, a.rows, a.maxlag
    Cn = S * Cs
    tabs = tables(torch, T, Cn, a.nt, a.layers, dev)
    models = tabs["models"]
    torch.cuda.synchronize()
    site_of, ids = np.arange(Cn) // Cs, np.arange(Cn)
    feats = site_features(np.random.RandomState(3), S)
    site_rows = torch.from_numpy(np.tile(site_of, T).astype(np.int32)).to(dev)

    def form_a():
        out = D.chain_feature_series(models, feats, site_of, engine=eng, nsites=S)
        torch.cuda.synchronize()
        return out

    def form_b():
        got = posterior_classes(models.reshape(T * Cn, -1), {"all": []}, site=site_rows, features=feats, engine=eng, nsites=S,
                                return_columns=True)
        cols = torch.stack([got["columns"][lb].reshape(T, Cn) for lb in labels], dim=2)
        nan = torch.isnan(cols)
        value, present = torch.where(nan, torch.zeros_like(cols), cols), (~nan).to(torch.float32)
        missing = nan.sum(dim=0).cpu().numpy().astype(np.int64)
        torch.cuda.synchronize()
        return value, present, missing

    labels = D.chain_feature_series(models[:64, :Cs], feats, site_of[:Cs], engine=eng, nsites=S)[3]      # warm-up
    form_b_small = posterior_classes(models[:64].reshape(64 * Cn, -1), {"all": []}, site=site_rows[:64 * Cn], features=feats, engine=eng,
                                     nsites=S, return_columns=True)
    del form_b_small
    if a.trace:
        for _ in range(2):
            form_a()
            form_b()
        return
    ra, t_form_a = timed(form_a, a.reps)
    rb, t_form_b = timed(form_b, a.reps)
    assert torch.equal(ra[0].view(torch.int64), rb[0].view(torch.int64)), "B's value table is not A's bits"
    assert torch.equal(ra[1].view(torch.int32), rb[1].view(torch.int32)), "B's present table is not A's bits"
    assert np.array_equal(ra[2], rb[2])
    present_share = {lb: float(1.0 - ra[2][:, q].sum() / float(T * Cn)) for q, lb in enumerate(labels)}
    # downstream of the tables, common to both routes
    _, t_conv = timed(lambda: D.feature_convergence(ra[0], ra[1], ra[2], site_of, L, engine=eng, labels=labels), a.reps)
    del rb
    small = {k: v[:64, :Cs] for k, v in tabs.items()}
    D.diagnose(small, site_of[:Cs], ids[:Cs], maxlag=8, engine=eng, features={k: (v[0],) + tuple(np.atleast_1d(x)[:1] for x in v[1:])
                                                                              for k, v in feats.items()})
    r_plain, t_plain = timed(lambda: D.diagnose(tabs, site_of, ids, maxlag=L, engine=eng), a.reps)
    r_feat, t_feat = timed(lambda: D.diagnose(tabs, site_of, ids, maxlag=L, engine=eng, features=feats), a.reps)
    f0 = r_feat[0]["features"]
    met = t_form_a["best_s"] <= t_form_b["best_s"] + t_form_b["spread_s"]
    res = dict(sites=S, chains_per_site=Cs, rows=T, layers_max=a.layers, dtype="float32", maxlag=L, features=len(feats), columns=len(labels),
               labels=labels, kinds=[f[0] for f in feats.values()],
               A_chain_feature_series=t_form_a, B_posterior_classes_columns_reshaped=t_form_b,
               bar="A's column-forming stage no slower than B's by more than the spread of B's repeats", bar_met=bool(met),
               forming_speedup_A_over_B=t_form_b["best_s"] / t_form_a["best_s"], same_bits=True,
               feature_convergence_on_the_tables=t_conv, diagnose_without_features=t_plain, diagnose_with_features=t_feat,
               whole_B_est_s=t_form_b["best_s"] + t_conv["best_s"], whole_A_s=t_form_a["best_s"] + t_conv["best_s"],
               share_of_rows_with_the_column=present_share,
               site0=dict(complete=[bool(v) for v in f0["complete"]], probability=[float(v) for v in f0["probability"]],
                          rhat=[float(v) for v in f0["rhat"]], ess=[float(v) for v in f0["ess"]], mean=[float(v) for v in f0["mean"]],
                          mcse_mean=[float(v) for v in f0["mcse_mean"]]),
               per_kernel_times="in profiles/chain_diag_features_kernels.txt: one rocprofv3 --kernel-trace --stats run of --trace")
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
