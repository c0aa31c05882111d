"""The restatement of the chain diagnostics (tests/diag_ref.py) and bayhunter_amd.diagnostics.convergence / outlier_chains held to
what is known in closed form.  No GPU: the tables come from the restatement."""
import math
import os

import numpy as np
import pytest

import diag_ref as R
from bayhunter_amd import diagnostics as D
from bayhunter_amd import results


def alternating(T, C=1):
    x = np.where(np.arange(T) % 2 == 0, 1.0, -1.0)
    return np.repeat(x[:, None], C, axis=1)


def both(tab, site_of_chain, exclude=()):
    """convergence() of the package, and the restatement per site and column in the same layout"""
    got = D.convergence(tab, site_of_chain, exclude)
    ref = []
    for s in range(len(got)):
        chains = [c for c in range(len(site_of_chain)) if site_of_chain[c] == s and c not in exclude]
        ref.append([R.convergence(tab, chains, q) for q in range(tab["x0"].shape[1])])
    return got, ref


def close(a, b, rtol=1e-12):
    a, b = float(a), float(b)
    return (math.isnan(a) and math.isnan(b)) or a == b or abs(a - b) <= rtol * abs(b)


def assert_same(got, ref):
    for g, rs in zip(got, ref):
        for q, r in enumerate(rs):
            for k in ("rhat", "ess", "tau"):
                assert close(g[k][q], r[k]), (k, q, g[k][q], r[k])
            assert g["cut"][q] == r["cut"] and bool(g["ess_truncated"][q]) == r["truncated"] and bool(g["constant"][q]) == r["constant"]
            for j in range(len(g["chains"])):
                for k in ("mean", "std", "chain_tau"):
                    assert close(g[k][j, q], r[k][j]), (k, j, q)


@pytest.mark.parametrize("T", [2, 8, 64, 1000])
def test_alternating_series_has_its_closed_lag_sums(T):
    tab = R.tables(alternating(T), L=T + 3)
    assert tab["x0"][0, 0] == 1.0 and tab["s1"][0, 0] == -float(T)
    for k in range(T + 4):
        assert tab["p"][0, 0, k] == ((-1.0) ** k * (T - k) if k < T else 0.0)
    h = T // 2
    assert tab["m2a"][0, 0] == tab["m2b"][0, 0] == (0.0 if T == 2 else float(h))     # (every other T here has an even h)


@pytest.mark.parametrize("m", [1, 2, 5])
def test_identical_chains_give_the_closed_rhat_and_the_capped_ess(m):
    """m identical chains whose halves are identical: B = 0, rhat = sqrt((h-1)/h).  The alternating series is anticorrelated, its
    first Geyer pair is negative: cut 0, tau = -1, and the ESS is the cap m n log10(m n)."""
    T = 64
    tab = R.tables(alternating(T, m), L=10)
    got, ref = both(tab, [0] * m)
    assert_same(got, ref)
    h = T // 2
    assert close(got[0]["rhat"][0], math.sqrt((h - 1) / h), 1e-15)
    assert got[0]["cut"][0] == 0 and got[0]["tau"][0] == -1.0 and not got[0]["ess_truncated"][0]
    assert close(got[0]["ess"][0], m * T * math.log10(m * T), 1e-14)
    assert np.all(got[0]["mean"] == 0.0) and np.allclose(got[0]["std"], math.sqrt(T / (T - 1.0)), rtol=1e-15, atol=0)


def test_geyer_cut_monotone_step_and_truncation_on_a_hand_built_table():
    rho = [1.0, 0.5, 0.1, 0.1, 0.3, 0.2, 0.05, -0.1, 0.4, 0.4]      # pairs 1.5, 0.2, 0.5, -0.05, 0.8
    for f in (R.geyer, D.geyer_tau):
        tau, cut, trunc = f(rho)
        assert cut == 3 and not trunc and close(tau, -1 + 2 * (1.5 + 0.2 + 0.2), 1e-15)     # 0.5 lowered to 0.2; nothing behind the cut
        tau, cut, trunc = f(rho[:6])
        assert cut == 3 and trunc and close(tau, -1 + 2 * (1.5 + 0.2 + 0.2), 1e-15)         # positive up to the lag limit
        tau, cut, trunc = f(rho[:7])                                                           # an odd count: the last lag has no pair
        assert cut == 3 and trunc
        tau, cut, trunc = f([1.0, -1.0])                                                       # a pair of exactly zero is cut
        assert cut == 0 and not trunc and tau == -1.0
        tau, cut, trunc = f([1.0])                                                             # no pair at all
        assert math.isnan(tau) and cut == 0 and trunc


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5])
def test_short_series_give_nan_and_no_error(T):
    rs = np.random.RandomState(T)
    x = rs.standard_normal((T, 3, 2))
    tab = R.tables(x, L=3)
    got, ref = both(tab, [0, 0, 1])
    assert_same(got, ref)
    for g in got:
        if T < 4:
            assert np.all(np.isnan(g["rhat"])) and np.all(np.isnan(g["ess"]))
        else:
            assert np.all(np.isfinite(g["rhat"])) and np.all(np.isfinite(g["ess"]))
        assert np.all(np.isfinite(g["mean"])) and (T == 1 or np.all(np.isfinite(g["std"])))


def test_constant_columns_single_chains_and_excluded_chains():
    rs = np.random.RandomState(3)
    x = rs.standard_normal((40, 4, 3))
    x[:, :, 1] = np.array([1.5, 1.5, 2.5, -3.0])           # every chain constant (not the same constant)
    x[:, 0, 2] = 7.0                                        # one stuck chain among moving ones
    tab = R.tables(x, L=20)
    assert np.all(tab["p"][:, 1] == 0.0) and np.all(tab["m2a"][:, 1] == 0.0) and np.all(tab["s1"][:, 1] == 0.0)
    got, ref = both(tab, [0, 0, 0, 1])                      # site 1: m = 1
    assert_same(got, ref)
    assert list(got[0]["constant"]) == [False, True, False] and list(got[1]["constant"]) == [False, True, False]
    assert np.isnan(got[0]["rhat"][1]) and np.isnan(got[0]["ess"][1]) and np.isnan(got[1]["rhat"][1])
    assert np.isfinite(got[1]["rhat"][0]) and np.isfinite(got[1]["ess"][0])                # m = 1 works
    assert np.isnan(got[0]["chain_tau"][0, 2]) and got[0]["std"][0, 2] == 0.0 and np.isfinite(got[0]["chain_tau"][1, 2])
    assert got[0]["rhat"][2] > 1.1                          # the stuck chain shows
    got, ref = both(tab, [0, 0, 0, 1], exclude=(0, 3))
    assert_same(got, ref)
    assert list(got[0]["chains"]) == [1, 2] and got[1]["chains"].size == 0 and np.all(np.isnan(got[1]["rhat"]))
    assert got[0]["rhat"][2] < 1.1


def write_likes(path, likes, ids):
    os.makedirs(path, exist_ok=True)
    for j, c in enumerate(ids):
        np.save(os.path.join(path, "c%03d_p2likes.npy" % c), likes[:, j])


@pytest.mark.parametrize("branch,levels,dev", [
    ("positive", [100.0, 99.0, 94.0, 96.0, 80.0], 0.05),
    ("negative", [-100.0, -101.0, -106.0, -104.0, -130.0], 0.05),
    ("zero", [0.0, -5.0, -1.0, 0.0, -50.0], 0.05),
    ("at dev", [4.0, 3.0, 2.9990234375, 3.5, 4.0], 0.25),        # 1 - 3/4 is exactly dev: no outlier, the rule is strict
])
def test_outlier_chains_is_the_reference_rule_per_site(tmp_path, branch, levels, dev):
    rs = np.random.RandomState(11)
    T, ids = 41 if branch != "negative" else 40, [0, 1, 2, 5, 7]
    likes = np.zeros((T, 2 * len(levels)), np.float32)
    for j, lv in enumerate(levels):              # the median of every chain is its level, exactly
        noise = rs.standard_normal(T // 2).astype(np.float32)
        col = np.concatenate((lv + np.abs(noise) * 0.5, lv - np.abs(noise) * 0.5, [lv] * (T - 2 * (T // 2)))).astype(np.float32)
        if T % 2 == 0:
            col[0], col[T // 2] = lv, lv         # the two middle values
        likes[:, j] = rs.permutation(col)
        likes[:, len(levels) + j] = likes[::-1, j] * np.float32(2.0 if branch != "zero" else 1.0)
    assert np.array_equal(np.median(likes[:, :len(levels)], axis=0), np.array(levels, np.float32))
    site_of = [0] * len(levels) + [1] * len(levels)
    outl, scores = D.outlier_chains(likes, site_of, dev=dev)
    for s in range(2):
        cols = np.flatnonzero(np.array(site_of) == s)
        path = str(tmp_path / ("site%d" % s))
        write_likes(path, likes[:, cols], ids)
        ref = results.get_outliers(path, dev=dev)
        assert np.array_equal(np.array(ids)[outl[s] - cols[0]], ref.astype(int))
        if ref.size:
            txt = [ln.split() for ln in open(os.path.join(path, "outliers.dat")) if not ln.startswith("#")]
            assert [int(t[0]) for t in txt] == list(ref.astype(int)) and ["%.3f" % v for v in scores[s]] == [t[1] for t in txt]
    if branch == "positive":
        assert list(outl[0]) == [2, 4]
    elif branch == "negative":
        assert list(outl[0]) == [2, 4]
    elif branch == "zero":
        assert list(outl[0]) == [] and list(outl[1]) == []
    else:
        assert list(outl[0]) == [2]


def test_ar1_chains_meet_the_estimators_conditions():
    """4 chains of AR(1), phi = 0.9, T = 20000: ESS / (m T) within a factor 2 of (1 - phi) / (1 + phi) and rhat < 1.01; one chain
    shifted by 3 sigma gives rhat > 1.1.  Conditions on the estimator, on a fixed seed."""
    phi, T, m = 0.9, 20000, 4
    x = R.ar1(np.random.RandomState(20261018), T, m, phi)
    tab = R.tables(x, L=150)
    got, ref = both(tab, [0] * m)
    assert_same(got, ref)
    g = got[0]
    want = (1 - phi) / (1 + phi)
    assert want / 2 < g["ess"][0] / (m * T) < want * 2 and g["rhat"][0] < 1.01 and not g["ess_truncated"][0]
    assert np.all(np.abs(g["chain_tau"][:, 0] - (1 + phi) / (1 - phi)) < 0.5 * (1 + phi) / (1 - phi))
    x[:, 2] += 3.0 / math.sqrt(1 - phi * phi)
    got = D.convergence(R.tables(x, L=150), [0] * m)
    assert got[0]["rhat"][0] > 1.1
