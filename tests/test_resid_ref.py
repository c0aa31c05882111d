"""tests/resid_ref.py, the restatement of include/bh_engine_posterior_resid.h, held to exact rational arithmetic, to hand cases and
to a statistical anchor: AR(1) noise of known r and sigma gives the acf_1 and the sigma_ratio the README promises."""
from fractions import Fraction

import numpy as np
import pytest

import resid_ref as RR

SIZES = (1, 2, 63, 64, 65, 130)


def exact_sum(terms):
    return sum((Fraction(float(x)) for x in terms), Fraction(0))


@pytest.mark.parametrize("n", SIZES)
def test_sums_against_exact_rationals(n):
    """every sum within n * 2^-53 * sum |terms| of the exact sum of the same rounded terms (each of the at most n - 1 additions a
    term goes through loses at most 2^-53 of a partial sum, which is at most sum |terms| (1 + 2^-53)^n)"""
    rs = np.random.RandomState(n)
    e = rs.normal(0.0, 0.05, n) * 10.0 ** rs.randint(-3, 4, n)
    g = rs.uniform(0.3, 1.0, n)
    u = e * g
    L = 8
    bound = lambda terms: n * 2.0 ** -53 * float(exact_sum(np.abs(terms)))
    assert abs(Fraction(RR.strand_sum(e)) - exact_sum(e)) <= Fraction(bound(e))
    sq = e * e
    assert abs(Fraction(RR.strand_sum(sq)) - exact_sum(sq)) <= Fraction(bound(sq))
    A = RR.lag_sums(u, L)
    assert len(A) == L + 1
    for l in range(L + 1):
        terms = u[:max(n - l, 0)] * u[l:] if l < n else np.zeros(0)
        assert abs(Fraction(A[l]) - exact_sum(terms)) <= Fraction(bound(terms)), (n, l)
        if l >= n:
            assert A[l] == 0.0


@pytest.mark.parametrize("n", SIZES)
def test_columns_follow_their_sums(n):
    """the columns are the stated single operations on the sums"""
    rs = np.random.RandomState(100 + n)
    yobs = rs.normal(0, 1, n)
    ymod = yobs + rs.normal(0, 0.05, n)
    L = 4
    c = RR.columns(ymod, yobs, 0.4, 0.05, L)
    e = ymod - yobs
    A = RR.lag_sums(e, L)
    assert c[0] == RR.strand_sum(e) / n
    assert c[1] == np.sqrt(RR.strand_sum(e * e) / n) and c[1] == np.sqrt(A[0] / n)
    assert c[2] == np.sqrt(A[0] / n) / 0.05 and c[3] == 0.4
    for l in range(1, L + 1):
        if l < n:
            assert c[RR.FIXED + l - 1] == A[l] / A[0]
        else:
            assert np.isnan(c[RR.FIXED + l - 1])
    assert (c[4] == A[1] / A[0] - 0.4) if n > 1 else np.isnan(c[4])
    assert np.isfinite(c[~np.isnan(c)]).all()


def test_alternating_residual():
    c = RR.columns([1.0, -1.0, 1.0, -1.0], np.zeros(4), 0.25, 2.0, 3)
    assert c[0] == 0.0 and c[1] == 1.0 and c[2] == 0.5 and c[3] == 0.25
    assert c[5] == -0.75 and c[6] == 0.5 and c[7] == -0.25 and c[4] == -1.0


def test_zero_residual_gives_nan_quotients():
    y = np.array([0.3, -1.5, 2.0, 7.0, 0.1])
    c = RR.columns(y, y, 0.5, 0.1, 3)
    assert c[0] == 0.0 and c[1] == 0.0 and c[2] == 0.0 and c[3] == 0.5
    assert np.isnan(c[4]) and np.isnan(c[5:]).all()


def test_lags_beyond_the_samples_are_masked():
    c = RR.columns([1.0, 2.0, 4.0], np.zeros(3), 0.0, 1.0, 5)
    assert c[5] == (1.0 * 2.0 + 2.0 * 4.0) / 21.0 and c[6] == 4.0 / 21.0 and np.isnan(c[7:]).all()
    one = RR.columns([3.0], [1.0], 0.1, 0.5, 2)
    assert one[0] == 2.0 and one[1] == 2.0 and one[2] == 4.0 and one[3] == 0.1 and np.isnan(one[4:]).all()


def test_sigma_zero_and_bad_noise_values():
    yobs = np.zeros(4)
    ymod = np.array([0.1, -0.2, 0.3, 0.05])
    ok = RR.columns(ymod, yobs, 0.3, 0.1, 2)
    z = RR.columns(ymod, yobs, 0.3, 0.0, 2)
    assert np.isnan(z[2]) and np.array_equal(np.delete(z, 2), np.delete(ok, 2))
    neg = RR.columns(ymod, yobs, 0.3, -0.1, 2)
    assert neg[2] == -ok[2]                                # (finite: left for the reader; only what is not finite is masked)
    bad = RR.columns(ymod, yobs, np.inf, np.nan, 2)
    assert np.isnan(bad[2:5]).all() and np.array_equal(bad[:2], ok[:2]) and np.array_equal(bad[5:], ok[5:])
    assert np.isnan(RR.columns(ymod, yobs, 0.3, 0.1, 2, err=3)).all()
    assert np.isnan(RR.columns([], [], 0.3, 0.1, 2)).all()


def test_weights_enter_the_lag_sums_only():
    rs = np.random.RandomState(5)
    yobs, ymod = rs.normal(0, 1, 40), rs.normal(0, 1, 40)
    g = 1.0 / np.sqrt(rs.uniform(1.0, 4.0, 40))
    c, c1 = RR.columns(ymod, yobs, 0.0, 0.2, 3, g=g), RR.columns(ymod, yobs, 0.0, 0.2, 3)
    assert np.array_equal(c[:2], c1[:2]) and c[2] != c1[2] and (c[5:] != c1[5:]).all()
    u = (ymod - yobs) * g
    A = RR.lag_sums(u, 3)
    assert c[2] == np.sqrt(A[0] / 40) / 0.2 and c[6] == A[2] / A[0]
    assert np.array_equal(RR.columns(ymod, yobs, 0.0, 0.2, 3, g=np.ones(40)), c1)


def test_the_set_places_slots_and_masks():
    rs = np.random.RandomState(9)
    ncol = np.array([[3, 2], [2, 0]])
    yobs = rs.normal(0, 1, (2, 5))
    ymod = rs.normal(0, 1, (3, 5))
    noise = np.array([[0.1, 0.2, 0.3, 0.4]] * 3, np.float32)
    v = RR.resid_set(ymod, [0, 0, 1], [0, 1, 0], ncol, yobs, noise, 2)
    assert v.shape == (3, 14) and np.isnan(v[2]).all() and np.isnan(v[1, 7:]).all()
    assert np.array_equal(v[0, 7:], RR.columns(ymod[0, 3:5], yobs[0, 3:5], np.float32(0.3), np.float32(0.4), 2), equal_nan=True)
    assert np.array_equal(v[1, :7], RR.columns(ymod[1, :2], yobs[1, :2], np.float32(0.1), np.float32(0.2), 2), equal_nan=True)
    assert v[0, 3] == float(np.float32(0.1)) and np.array_equal(RR.column_blocks(ncol), [0, 3, 5])


def test_acf_model():
    assert np.array_equal(RR.acf_model("exp", 0.5, 3), [0.5, 0.25, 0.125])
    assert np.array_equal(RR.acf_model("gauss", 0.5, 3), [0.5, 0.5 ** 4, 0.5 ** 9])
    assert not RR.acf_model("nocorr", 0.5, 3).any() and not RR.acf_model("nocorr_scalederr", 0.5, 3).any()


def test_ar1_noise_is_recognised():
    """AR(1) noise with r = 0.9, sigma = 0.05, n = 2000, 200 rows: per row acf_1 has sd ~ sqrt((1 - r^2) / n) ~ 0.0097 and bias
    ~ -(1 + 3 r) / n ~ -0.002, so the mean over the rows lies within 0.01 of 0.9; the mean sigma_ratio within 0.02 of 1"""
    r, sigma, n, rows = 0.9, 0.05, 2000, 200
    rs = np.random.RandomState(20261020)
    w = rs.normal(0.0, 1.0, (rows, n))
    x = np.empty((rows, n))
    x[:, 0] = w[:, 0]
    for i in range(1, n):
        x[:, i] = r * x[:, i - 1] + np.sqrt(1.0 - r * r) * w[:, i]
    x *= sigma
    yobs = rs.normal(0, 1, n)
    c = np.array([RR.columns(yobs + x[k], yobs, r, sigma, 3) for k in range(rows)])
    assert abs(c[:, 5].mean() - r) <= 0.01, c[:, 5].mean()
    assert abs(c[:, 2].mean() - 1.0) <= 0.02, c[:, 2].mean()
    assert abs(c[:, 4].mean()) <= 0.01 and abs(c[:, 6].mean() - r * r) <= 0.02
