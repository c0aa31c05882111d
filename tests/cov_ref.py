"""A restatement of the posterior covariance (include/bh_engine_posterior_cov.h, bayhunter_amd.posterior.posterior_covariance) in
Python integers and Fractions, on posterior_ref.interp and moho_ref: the L / X0 / Y rule, the limb sums, N_ij, and mean, cov and
corr as exact rationals.  The GPU tests' oracle; tests/test_cov_ref.py holds it against numpy.cov and numpy.corrcoef.

The rule, per column over the rows used (a row with NaN in any scalar column is used by no column):
  low = the exponent of the lowest set bit of any value;  L = the smallest exponent >= low with
  rint(max 2^-L) - rint(min 2^-L) < 2^28 (rint: to nearest, ties to even);  exact = (L == low);  X0 = rint(min 2^-L);
  Y = rint(v 2^-L) - X0;  a column of zeros only has L = 0, X0 = 0, exact.
  Y = H 2^14 + Lo;  raw_ij = (sum H_i H_j, sum (H_i Lo_j + Lo_i H_j), sum Lo_i Lo_j) for i <= j;  s_i = sum Y_i;
  S_ij = raw0 2^28 + raw1 2^14 + raw2;  N_ij = n S_ij - s_i s_j;
  mean_i = (s_i / n + X0_i) 2^L_i;  cov_ij = N_ij / n^2 2^(L_i + L_j);  corr_ij = N_ij / sqrt(N_ii N_jj).
"""
from fractions import Fraction
import math

import numpy as np

import posterior_ref as R

LIMB = 14
WIDTH = 1 << (2 * LIMB)


def low_bit(v):
    """the exponent of the lowest set bit of a float (None for 0)"""
    f = Fraction(float(v))
    if f == 0:
        return None
    num = abs(f.numerator)
    return ((num & -num).bit_length() - 1) - (f.denominator.bit_length() - 1)


def low_bits(col):
    """low_bit of every non-zero value of a float64 array, with numpy: the mantissa as a 53-bit integer, its trailing zeros"""
    v = np.asarray(col, np.float64)
    m, e = np.frexp(v[v != 0])
    M = np.abs(np.ldexp(m, 53)).astype(np.int64)
    return e.astype(np.int64) - 53 + np.log2((M & -M).astype(np.float64)).astype(np.int64)


def rint_scaled(v, L):
    """rint(v 2^-L) as a Python integer: exact scaling, to nearest, ties to even (Fraction.__round__)"""
    return round(Fraction(float(v)) / Fraction(2) ** L)


def column_scale(col):
    """(L, X0, exact) of the finite values of one column"""
    col = np.asarray(col, np.float64)
    lows = low_bits(col)
    if not lows.size:
        return 0, 0, 1
    low, mn, mx = int(lows.min()), col.min(), col.max()
    L = low
    while rint_scaled(mx, L) - rint_scaled(mn, L) >= WIDTH:
        L += 1
    return L, rint_scaled(mn, L), int(L == low)


def table(models, dep, scalars=None):
    """(V [n, P] float64 of the rows used, masked): the vs of every kept row at dep, then the scalar columns (float64 [Nkept, Qc],
    one row per kept row, NaN = no value); rows with NaN in a scalar column are left out"""
    dep = np.asarray(dep, np.float64)
    vsi = R.interp(models, dep) if dep.size else np.zeros((int(R.split(np.asarray(models))[1].sum()), 0))
    if scalars is None:
        return vsi, 0
    scalars = np.asarray(scalars, np.float64).reshape(len(vsi), -1)
    ok = ~np.isnan(scalars).any(1)
    return np.concatenate((vsi, scalars), axis=1)[ok], int((~ok).sum())


def pairs(P):
    return [(i, j) for i in range(P) for j in range(i, P)]


def integers(V):
    """the integers of one site's table V [n, P]: dict of n, L, x0, exact [P], Y (int64 [n, P]), s [P] and raw [P (P + 1) / 2][3]
    as Python integers.  rint(v 2^-L) is formed with numpy.ldexp and numpy.rint on float64 -- both exact here (a power-of-two
    scaling, and the rounding rule itself); the scale comes from column_scale's rationals."""
    V = np.asarray(V, np.float64)
    n, P = V.shape
    L, x0, exact = [0] * P, [0] * P, [1] * P
    Y = np.zeros((n, P), np.int64)
    for j in range(P if n else 0):
        L[j], x0[j], exact[j] = column_scale(V[:, j])
        X = np.rint(np.ldexp(V[:, j], -L[j]))
        Y[:, j] = np.array([int(x) - x0[j] for x in X], np.int64)
        assert Y[:, j].min() >= 0 and Y[:, j].max() < WIDTH
    H, Lo = Y >> LIMB, Y & ((1 << LIMB) - 1)                  # int64 products and sums: below n 2^29, exact
    hh, hl, ll = H.T @ H, H.T @ Lo, Lo.T @ Lo
    raw = [[int(hh[i, j]), int(hl[i, j]) + int(hl[j, i]), int(ll[i, j])] for i, j in pairs(P)]
    return dict(n=n, L=L, x0=x0, exact=exact, Y=Y, s=[int(v) for v in Y.sum(0)], raw=raw)


def numerators(n, s, raw):
    """N [P][P] (Python integers, symmetric): N_ij = n S_ij - s_i s_j"""
    P = len(s)
    N = [[0] * P for _ in range(P)]
    for (i, j), (r0, r1, r2) in zip(pairs(P), raw):
        S = (int(r0) << (2 * LIMB)) + (int(r1) << LIMB) + int(r2)
        N[i][j] = N[j][i] = n * S - int(s[i]) * int(s[j])
    return N


def two(e):
    return Fraction(2) ** int(e)


def finish(n, L, x0, s, raw):
    """(mean [P], cov [P][P], N [P][P]) as exact rationals / integers; corr_ij is N_ij / sqrt(N_ii N_jj) (within_ulp_corr)"""
    P = len(s)
    N = numerators(n, s, raw)
    mean = [(Fraction(int(s[i]), n) + int(x0[i])) * two(L[i]) for i in range(P)]
    cov = [[Fraction(N[i][j], n * n) * two(L[i] + L[j]) for j in range(P)] for i in range(P)]
    return mean, cov, N


def ulp(x):
    return Fraction(float(np.spacing(abs(np.float64(x)))))


def within_ulp(x, exact, k=1):
    """|x - exact| <= k ulp(x), exact a Fraction"""
    return abs(Fraction(float(x)) - exact) <= k * ulp(x)


def _cmp_sqrt(x, N, D):
    """sign of x sqrt(D) - N for a Fraction x, integers N and D > 0"""
    if x == 0 or N == 0 or (x > 0) != (N > 0):
        return (x > 0) - (x < 0) if x != 0 else -((N > 0) - (N < 0))
    d = x * x * D - N * N                                     # the same sign on both sides: compare the squares
    sgn = (d > 0) - (d < 0)
    return sgn if x > 0 else -sgn


def within_ulp_corr(x, Nij, Nii, Njj, k=1):
    """|x - N_ij / sqrt(N_ii N_jj)| <= k ulp(x), decided in integers"""
    fx, u, D = Fraction(float(x)), k * ulp(x), Nii * Njj
    return _cmp_sqrt(fx - u, Nij, D) <= 0 <= _cmp_sqrt(fx + u, Nij, D)


def corr_float(N):
    """corr as float64 [P, P] from the integers with 200 bits of square root: NaN where N_ii = 0 -- for tolerances far above 1 ulp"""
    P = len(N)
    out = np.full((P, P), np.nan)
    for i in range(P):
        for j in range(P):
            if N[i][i] > 0 and N[j][j] > 0:
                out[i, j] = float(Fraction(N[i][j] << 200, math.isqrt((N[i][i] * N[j][j]) << 400)))
    return out


def check_finished(mean, cov, corr, n, L, x0, s, raw, k=1):
    """the finished float64 numbers of one site against the rationals of its integers: a list of complaints (empty = all within k ulp,
    corr's diagonal exactly 1 or NaN, constant columns 0 / NaN, both matrices symmetric bit for bit, n = 0 all NaN)"""
    P = len(s)
    mean, cov, corr = np.asarray(mean), np.asarray(cov), np.asarray(corr)
    bad = []
    if n == 0:
        if not (np.isnan(mean).all() and np.isnan(cov).all() and np.isnan(corr).all()):
            bad.append("n = 0 is not all NaN")
        return bad
    em, ec, N = finish(n, L, x0, s, raw)
    for m in (cov, corr):
        if not np.array_equal(m.view(np.uint64), m.T.copy().view(np.uint64)):
            bad.append("not symmetric on bits")
    for i in range(P):
        if not within_ulp(mean[i], em[i], k):
            bad.append("mean[%d] = %r, exact %r" % (i, mean[i], float(em[i])))
        for j in range(i, P):
            if not within_ulp(cov[i, j], ec[i][j], k):
                bad.append("cov[%d, %d] = %r, exact %r" % (i, j, cov[i, j], float(ec[i][j])))
            c = corr[i, j]
            if N[i][i] <= 0 or N[j][j] <= 0:
                if not np.isnan(c) or cov[i, j] != 0.0:
                    bad.append("constant column: corr[%d, %d] = %r, cov %r" % (i, j, c, cov[i, j]))
            elif i == j:
                if c != 1.0:
                    bad.append("corr[%d, %d] = %r on the diagonal" % (i, j, c))
            elif not (-1.0 <= c <= 1.0 and within_ulp_corr(c, N[i][j], N[i][i], N[j][j], k)):
                bad.append("corr[%d, %d] = %r" % (i, j, c))
    return bad
