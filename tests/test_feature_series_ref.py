"""CPU tests of the convergence numbers of structural features (bayhunter_amd/diagnostics.py: feature_convergence): the rule for rows
that lack a feature on rows made by hand, and what mcse_mean means on replicate synthetic runs.  The sums come from tests/diag_ref.py
(exact sums rounded once) in place of the GPU call; everything downstream is the package's own code."""
import numpy as np
import pytest

import diag_ref as R
import feature_series_ref as FS
from bayhunter_amd import diagnostics as D
from bayhunter_amd.posterior import check_features
from test_features_ref import row_of


@pytest.fixture
def host_sums(monkeypatch):
    """feature_convergence with the restatement's sums where the GPU's would be"""
    monkeypatch.setattr(D, "chain_series_stats", lambda values, maxlag, engine=None, sel=None: R.tables(np.asarray(values), int(maxlag)))


FEATURES = {"moho": ("above", 20.0, 50.0, 4.2), "lvz": ("drop", 0.0, 60.0, 0.5), "slow": ("vsmin", 0.0, 60.0),
            "nif": ("nifaces", 20.0, 50.0)}
LABELS = ["moho", "lvz.depth", "lvz.jump", "slow.value", "slow.depth", "nif"]
ML = 4
ROWS = dict(
    half=row_of([3.5], [], np.float64, ML),                          # n = 1: no interface, every interface kind lacking
    at_z0=row_of([3.0, 4.5], [20.0], np.float64, ML),                # an interface exactly at z0: strictly outside
    at_z1=row_of([3.0, 4.5], [50.0], np.float64, ML),                # ... exactly at z1
    inside=row_of([3.0, 4.5], [35.0], np.float64, ML),
    tie=row_of([3.0, 2.5, 2.5, 4.5], [5.0, 10.0, 30.0], np.float64, ML),   # tied vsmin layers; a drop of exactly -c
    drop=row_of([3.0, 2.25, 4.5], [8.0, 32.0], np.float64, ML))
# (moho, lvz.depth, lvz.jump, slow.value, slow.depth, nif), NaN where the row lacks the column
WANT = dict(half=(np.nan, np.nan, np.nan, 3.5, 0.0, 0.0), at_z0=(np.nan, np.nan, np.nan, 3.0, 0.0, 0.0),
            at_z1=(np.nan, np.nan, np.nan, 3.0, 0.0, 0.0), inside=(35.0, np.nan, np.nan, 3.0, 0.0, 1.0),
            tie=(30.0, np.nan, np.nan, 2.5, 5.0, 1.0), drop=(32.0, 8.0, -0.75, 2.25, 8.0, 1.0))
CHAINS = [["inside", "tie", "drop", "half", "inside", "drop", "at_z0", "tie"],
          ["drop", "drop", "inside", "tie", "at_z1", "inside", "tie", "drop"],
          ["tie", "inside", "tie", "drop", "inside", "tie", "inside", "drop"]]


def hand_table():
    models = np.array([[ROWS[CHAINS[c][t]] for c in range(3)] for t in range(8)])
    kinds, par, labels = check_features(FEATURES, 1)
    assert labels == LABELS
    return models, kinds, par


def test_the_rule_on_rows_made_by_hand():
    models, kinds, par = hand_table()
    value, present, missing = FS.series_ref(models, kinds, par, np.zeros(3, int))
    for c in range(3):
        for t in range(8):
            want = np.array(WANT[CHAINS[c][t]])
            assert np.array_equal(present[t, c], (~np.isnan(want)).astype(np.float32)), (c, t)
            assert np.array_equal(value[t, c], np.where(np.isnan(want), 0.0, want)), (c, t)
            assert not np.signbit(value[t, c][np.isnan(want)]).any(), (c, t)      # +0.0 where the row lacks the column
    assert np.array_equal(missing, [[2, 6, 6, 0, 0, 0], [1, 5, 5, 0, 0, 0], [0, 6, 6, 0, 0, 0]])


def test_bookkeeping_and_the_linearised_series(host_sums):
    models, kinds, par = hand_table()
    site = np.zeros(3, int)
    value, present, missing = FS.series_ref(models, kinds, par, site)
    L = 3
    got = D.feature_convergence(value, present, missing, site, L, labels=LABELS)[0]
    idx = np.arange(3)
    tv, tp = R.tables(value, 0), R.tables(present, L)
    rule = FS.missing_rule(value, present, missing, idx, tv["x0"] + tv["s1"] / 8, tp["x0"] + tp["s1"] / 8)
    assert got["labels"] == LABELS and np.array_equal(got["chains"], idx) and np.array_equal(got["missing"], missing)
    assert np.array_equal(got["complete"], [False, False, False, True, True, True]) and np.array_equal(got["complete"], rule["complete"])
    assert np.array_equal(got["probability"], [21 / 24., 7 / 24., 7 / 24., 1.0, 1.0, 1.0])
    assert np.array_equal(got["mean"], rule["m"])
    # the conditional mean is the mean of the rows that have the column (the values are dyadic: exact)
    has = present.astype(bool)
    for q in range(6):
        assert abs(got["mean"][q] - value[:, :, q][has[:, :, q]].mean()) < 1e-14
    # R-hat, ESS and the rest are convergence() of x, and of the indicator under `presence`
    tx = R.tables(rule["x"], L)
    cx, cp = D.convergence(tx, site)[0], D.convergence(tp, site)[0]
    for k in ("rhat", "ess", "tau", "cut", "ess_truncated", "constant", "chain_tau"):
        assert np.array_equal(got[k], cx[k], equal_nan=True), k
        assert np.array_equal(got["presence"][k], cp[k], equal_nan=True), k
    assert sorted(got) == sorted(["labels", "chains", "missing", "complete", "probability", "presence", "mean", "mcse_mean", "rhat", "ess",
                                  "tau", "cut", "ess_truncated", "constant", "chain_tau"])
    assert sorted(got["presence"]) == sorted(list(cp) + ["mcse_probability"])
    assert np.array_equal(got["presence"]["constant"], [False, False, False, True, True, True])
    pq = np.where(rule["complete"], 1.0, rule["probability"])
    with np.errstate(all="ignore"):
        assert np.array_equal(got["mcse_mean"], FS.pooled_sd(tx, idx) / (pq * np.sqrt(cx["ess"])), equal_nan=True)
        assert np.array_equal(got["presence"]["mcse_probability"], FS.pooled_sd(tp, idx) / np.sqrt(cp["ess"]), equal_nan=True)
    # the pooled deviation is numpy's over the kept rows
    assert np.allclose(FS.pooled_sd(tx, idx), rule["x"].reshape(24, 6).std(axis=0, ddof=1), rtol=1e-13, atol=0)
    assert np.array_equal(D.pooled_sd(tx, idx), FS.pooled_sd(tx, idx))


def test_exclusions_and_a_column_no_kept_row_has(host_sums):
    models, kinds, par = hand_table()
    models[:, 2] = ROWS["half"]                # the third chain never has an interface
    site = np.array([0, 0, 1])
    kinds, par, _ = check_features(FEATURES, 2)
    value, present, missing = FS.series_ref(models, kinds, par, site)
    got = D.feature_convergence(value, present, missing, site, 3, exclude=[1])
    assert np.array_equal(got[0]["chains"], [0]) and np.array_equal(got[1]["chains"], [2]) and "labels" not in got[0]
    assert np.array_equal(got[0]["missing"], missing[[0]]) and np.array_equal(got[0]["probability"], [6 / 8., 2 / 8., 2 / 8., 1, 1, 1])
    g = got[1]
    assert np.array_equal(g["probability"], [0, 0, 0, 1, 1, 1]) and np.all(np.isnan(g["mean"][:3])) and np.all(g["constant"])
    assert np.array_equal(g["mean"][3:], [3.5, 0.0, 0.0]) and np.all(np.isnan(g["mcse_mean"])) and not g["complete"][:3].any()


def test_the_conditional_mean_and_the_order_of_rows_and_chains(host_sums):
    models, kinds, par = hand_table()
    site = np.zeros(3, int)
    value, present, missing = FS.series_ref(models, kinds, par, site)
    base = D.feature_convergence(value, present, missing, site, 3)[0]["mean"]
    rs = np.random.RandomState(3)
    for _ in range(4):                        # the rows of every chain in another order: the same bits (T cancels, the sums are exact)
        v, p = value.copy(), present.copy()
        for c in range(3):
            o = rs.permutation(8)
            v[:, c], p[:, c] = value[o, c], present[o, c]
        assert np.array_equal(D.feature_convergence(v, p, missing, site, 3)[0]["mean"], base)
    # the chains in another order: the sums over the chains are ascending, so only the value is the same, not by contract the bits
    o = np.array([2, 0, 1])
    other = D.feature_convergence(value[:, o], present[:, o], missing[o], site, 3)[0]["mean"]
    assert np.allclose(other, base, rtol=4e-16, atol=0)


def test_mcse_mean_predicts_the_spread_of_the_conditional_mean_over_replicates(host_sums):
    """150 replicate runs of 4 chains x 2000 rows: presence z > 0.5 of an AR(1) series z with phi = 0.9, value 35 + 2 AR(1)(0.8) +
    0.8 z.  The mean of the predicted mcse_mean over the replicates, divided by the standard deviation of the conditional mean across
    them, must lie in [0.8, 1.25]: an sd from 150 replicates carries 1 / sqrt(298) = 5.8 % relative error, three of those are about
    17 %, and the window adds an allowance for the bias of the ESS estimator.  Measured: 1.08 (and 0.92 for mcse_probability, which
    is printed, not asserted)."""
    nrep, Cn, T, L = 150, 4, 2000, 100
    rs = np.random.RandomState(20240607)
    z = R.ar1(rs, T, Cn * nrep, 0.9) * np.sqrt(1 - 0.81)          # unit variance
    w = R.ar1(rs, T, Cn * nrep, 0.8) * np.sqrt(1 - 0.64)
    present = (z > 0.5).astype(np.float32)
    value = np.where(z > 0.5, 35.0 + 2.0 * w + 0.8 * z, 0.0)
    site = np.zeros(Cn, int)
    means, mcse, prob, mcse_p = [], [], [], []
    for r in range(nrep):
        sl = slice(Cn * r, Cn * r + Cn)
        v, p = value[:, sl, None], present[:, sl, None]
        d = D.feature_convergence(v, p, (p == 0).sum(axis=0), site, L)[0]
        assert not d["complete"][0] and not d["ess_truncated"][0]
        means.append(d["mean"][0]); mcse.append(d["mcse_mean"][0]); prob.append(d["probability"][0])
        mcse_p.append(d["presence"]["mcse_probability"][0])
    ratio = np.mean(mcse) / np.std(means, ddof=1)
    ratio_p = np.mean(mcse_p) / np.std(prob, ddof=1)
    print("mcse_mean: predicted %.4f, empirical %.4f, ratio %.3f; mcse_probability ratio %.3f"
          % (np.mean(mcse), np.std(means, ddof=1), ratio, ratio_p))
    assert 0.8 <= ratio <= 1.25
