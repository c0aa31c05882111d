"""The normal scores (diagnostics.normal_quantile, rank_table), the restatement of the rank transform (tests/rank_ref.py) and the
rank-normalised numbers formed from it (diagnostics.rank_summary over diagnostics.convergence) held to what is known.  No GPU: the
rank tables come from the restatement, the sums from tests/diag_ref.py."""
import statistics

import numpy as np
import pytest

import diag_ref as R
import rank_ref as K
from bayhunter_amd import diagnostics as D


def quantile_points():
    """1e4 points: both tails down to 1e-12, a dyadic grid (p and 1 - p both exact), the edges of the central branch, the smallest
    rank arguments (1 - 3/8) / (N + 1/4) of pools of 1, 4 and 3.2e5"""
    rs = np.random.RandomState(1)
    tails = 10.0 ** -rs.uniform(0.0, 12.0, 2500)
    grid = np.arange(1, 4096) / 4096.0
    pts = np.concatenate((tails, 1.0 - tails, grid, [1e-12, 1.0 - 1e-12, 0.075, 0.925, 0.5, 0.5 - 2.0 ** -40, 0.5 + 2.0 ** -40],
                          [(1 - 0.375) / (N + 0.25) for N in (1, 4, 320000)], [1.0 - (1 - 0.375) / (N + 0.25) for N in (4, 320000)]))
    rest = rs.uniform(0.0, 1.0, 10000 - pts.size)
    return np.concatenate((pts, rest))


def test_normal_quantile_against_the_standard_library():
    """AS241's published relative accuracy is about 1e-16 and the standard library evaluates the same rational functions: 1e-15
    leaves one decade for the order of operations and the logarithm's last bit."""
    p = quantile_points()
    assert p.size == 10000 and p.min() <= 1e-12 and np.all((p > 0) & (p < 1))
    got = D.normal_quantile(p)
    inv = statistics.NormalDist().inv_cdf
    want = np.array([inv(float(v)) for v in p])
    rel = np.abs(got - want) / np.where(want == 0.0, 1.0, np.abs(want))
    print("largest relative difference", rel.max())
    assert rel.max() <= 1e-15
    assert D.normal_quantile(0.5) == 0.0 and D.normal_quantile(np.array([0.0, 1.0])).tolist() == [-np.inf, np.inf]
    assert np.all(np.isnan(D.normal_quantile(np.array([-0.1, 1.1, np.nan]))))
    assert D.normal_quantile(np.zeros((2, 3)) + 0.3).shape == (2, 3)


def test_normal_quantile_is_monotone_and_antisymmetric():
    """monotone over the sorted points; antisymmetric about 1/2, to the bound above, where 1 - p is exact (the dyadic grid and
    powers of two down to 2^-40: the subtraction 1 - (1 - p) inside the algorithm then returns p itself)"""
    p = np.unique(quantile_points())
    x = D.normal_quantile(p)
    assert np.all(np.diff(x) >= 0.0)
    for N in (1, 4, 1000, 320000):
        assert np.all(np.diff(D.rank_table(N)[2:]) > 0.0)
    dy = np.concatenate((np.arange(1, 4096) / 4096.0, 2.0 ** -np.arange(2.0, 41.0)))
    assert np.array_equal(1.0 - (1.0 - dy), dy)
    a, b = D.normal_quantile(dy), D.normal_quantile(1.0 - dy)
    rel = np.abs(a + b) / np.where(a == 0.0, 1.0, np.abs(a))
    print("largest relative asymmetry", rel.max())
    assert rel.max() <= 1e-15


def test_rank_table():
    for N in (1, 2, 7, 1000):
        zt = D.rank_table(N)
        assert zt.shape == (2 * N + 1,) and zt.dtype == np.float64 and np.all(np.isnan(zt[:2])) and np.all(np.isfinite(zt[2:]))
        assert zt[N + 1] == 0.0                         # the middle rank, and the score of a constant pool
        r = np.arange(2, 2 * N + 1)
        assert np.array_equal(zt[r], D.normal_quantile((r / 2.0 - 0.375) / (N + 0.25)))
    with pytest.raises(ValueError):
        D.rank_table(0)


def test_known_ranks():
    rs = np.random.RandomState(3)
    pool = rs.permutation(101).astype(np.float64) * 0.37 - 5.0
    assert np.array_equal(K.r2(pool), 2 * (np.argsort(np.argsort(pool)) + 1))                 # no ties: the ranks 1..N
    assert sorted(K.r2(pool) // 2) == list(range(1, 102))
    assert K.r2(np.array([1.0, 1.0, 2.0])).tolist() == [3, 3, 6]
    assert K.r2(np.array([-0.0, 0.0, -1.0]) + 0.0).tolist() == [5, 5, 2]
    z, zf, lo, hi = K.rank_pool(np.array([1.0, 1.0, 2.0]))
    zt = D.rank_table(3)
    assert np.array_equal(z, zt[[3, 3, 6]]) and np.array_equal(zf, zt[[3, 3, 6]])             # median 1: f = 0, 0, 1
    z, zf, lo, hi = K.rank_pool(np.array([5.0]))
    assert z.tolist() == [0.0] and zf.tolist() == [0.0] and lo.tolist() == [1.0] and hi.tolist() == [1.0]


def test_a_constant_pool_is_constant_and_nan():
    T, Cn = 50, 3
    x = np.full((T, Cn, 1), 2.5)
    z, zf, tail = K.rank_tables(x, np.zeros(Cn, int))
    assert np.all(z == 0.0) and np.all(zf == 0.0) and np.all(tail == 1.0)
    conv = [D.convergence(R.tables(t, 6), np.zeros(Cn, int))[0] for t in (z, zf, tail)]
    r = D.rank_summary(*conv)
    assert sorted(r) == sorted(("chains",) + D.RANK_FIELDS)
    for k in ("constant_bulk", "constant_fold", "constant_tail_lo", "constant_tail_hi"):
        assert r[k].tolist() == [True]
    for k in ("rhat_bulk", "rhat_fold", "rhat", "ess_bulk", "ess_tail_lo", "ess_tail_hi", "ess_tail"):
        assert np.isnan(r[k]).tolist() == [True], k


def test_tail_indicators_are_numpys_quantiles():
    """tail_lo, tail_hi against x <= numpy.quantile(pool, 0.05 / 0.95) on 200 random pools, every fourth of 3 distinct integers"""
    rs = np.random.RandomState(11)
    for i in range(200):
        N = int(rs.randint(1, 400))
        pool = rs.randint(3, 6, N).astype(np.float64) if i % 4 == 0 else rs.standard_normal(N) * 10.0 ** rs.randint(-2, 3)
        if i % 4 == 1:
            pool = np.round(pool, 1)             # some ties
        _, _, lo, hi = K.rank_pool(pool)
        assert np.array_equal(lo == 1.0, pool <= np.quantile(pool, 0.05)), (i, N)
        assert np.array_equal(hi == 1.0, pool <= np.quantile(pool, 0.95)), (i, N)


def rank_numbers(x, site_of_chain, L, exclude=()):
    """the dict `rank` of every site from the restatements alone: rank tables (rank_ref), their sums (diag_ref), convergence()"""
    site_of_chain = np.asarray(site_of_chain)
    group = np.where(np.isin(np.arange(site_of_chain.size), exclude), -1, site_of_chain)
    conv = [D.convergence(R.tables(t, L), site_of_chain, exclude) for t in K.rank_tables(x, group)]
    return [D.rank_summary(a, b, c) for a, b, c in zip(*conv)]


T_AR, L_AR = 1000, 100


def test_well_mixed_chains():
    x = R.ar1(np.random.RandomState(2021), T_AR, 4, 0.3)
    r = rank_numbers(x, np.zeros(4, int), L_AR)[0]
    print(r)
    assert r["rhat_bulk"][0] < 1.01 and r["rhat_fold"][0] < 1.01 and r["rhat"][0] == max(r["rhat_bulk"][0], r["rhat_fold"][0])
    assert 0 < r["ess_tail"][0] == min(r["ess_tail_lo"][0], r["ess_tail_hi"][0]) and r["ess_bulk"][0] > 400
    assert not r["constant_bulk"][0] and not r["constant_tail_lo"][0]


def test_a_chain_of_another_spread_shows_in_the_folded_rhat_only():
    x = R.ar1(np.random.RandomState(2021), T_AR, 4, 0.3)
    x[:, 2] = (x[:, 2] - x[:, 2].mean()) * 3.0 + np.delete(x, 2, axis=1).mean()       # 3 x the spread, the same mean
    r = rank_numbers(x, np.zeros(4, int), L_AR)[0]
    plain = D.convergence(R.tables(x, L_AR), np.zeros(4, int))[0]
    print(r["rhat_bulk"], r["rhat_fold"], plain["rhat"])
    assert r["rhat_fold"][0] > r["rhat_bulk"][0] and r["rhat_fold"][0] > 1.05 and plain["rhat"][0] < 1.01
    assert r["rhat"][0] == r["rhat_fold"][0]


def test_a_shifted_heavy_tailed_chain_shows_in_the_bulk_rhat():
    x = np.random.RandomState(5).standard_cauchy((T_AR, 4))
    y = x.copy()
    y[:, 1] += 2.0
    a = rank_numbers(x, np.zeros(4, int), L_AR)[0]
    b = rank_numbers(y, np.zeros(4, int), L_AR)[0]
    print(a["rhat_bulk"], b["rhat_bulk"])
    assert b["rhat_bulk"][0] > a["rhat_bulk"][0] and b["rhat_bulk"][0] > 1.05 and a["rhat_bulk"][0] < 1.01


def test_sites_exclusions_and_nan_propagation():
    """two interleaved sites and an excluded chain: every site's numbers are those of its kept chains alone; a site whose kept
    chains never leave one value has NaN in rhat and ess_tail while the other site's stay finite"""
    x = R.ar1(np.random.RandomState(9), 200, 5, 0.5)
    x[:, 1] = 7.0
    x[:, 3] = 7.0
    site = np.array([0, 1, 0, 1, 0])
    both = rank_numbers(x, site, 20, exclude=(4,))
    alone = rank_numbers(x[:, [0, 2]], np.zeros(2, int), 20)[0]
    assert both[0]["chains"].tolist() == [0, 2] and both[1]["chains"].tolist() == [1, 3]
    for k in D.RANK_FIELDS:
        assert np.array_equal(both[0][k], alone[k], equal_nan=True), k
    assert np.isfinite(both[0]["rhat"][0]) and np.isfinite(both[0]["ess_tail"][0])
    assert np.isnan(both[1]["rhat"][0]) and np.isnan(both[1]["ess_tail"][0]) and both[1]["constant_bulk"][0]
    a = dict(chains=np.arange(2), rhat=np.array([1.0, np.nan]), ess=np.array([5.0, 6.0]), ess_truncated=np.zeros(2, bool),
             constant=np.zeros(2, bool))
    t = dict(a, ess=np.array([3.0, np.nan, 9.0, 2.0]), ess_truncated=np.zeros(4, bool), constant=np.zeros(4, bool))
    r = D.rank_summary(a, dict(a, rhat=np.array([1.5, 1.2])), t)
    assert r["rhat"][0] == 1.5 and np.isnan(r["rhat"][1]) and np.isnan(r["ess_tail"][0]) and r["ess_tail"][1] == 2.0
