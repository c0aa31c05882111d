"""The restatement of the posterior covariance (tests/cov_ref.py) against numpy.cov and numpy.corrcoef on the golden rows, and the
library's bh_posterior_cov_finish (include/bh_engine_posterior_cov.h: pure host code, loaded without a GPU) against the exact
rationals on integers that stress its 128-bit arithmetic.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
import cov_ref as CR

KEYS = ("f32", "f64of32", "f64")
U = 2.0 ** -53
M28 = (1 << 28) - 1
FILL = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def G():
    return golden("posterior_golden.npz")


def test_low_bits_of_the_vector_form_are_the_rationals():
    rs = np.random.RandomState(0)
    v = np.concatenate((rs.uniform(-5, 5, 200), rs.uniform(-5, 5, 50).astype(np.float32),
                        [0.0, 1.0, 3.0 + 2.0 ** -40, 5e-324, 2.0 ** -1060 * 3, -7.5, 1e300, -0.0]))
    assert [CR.low_bit(x) for x in v if x != 0] == list(CR.low_bits(v))


def test_the_scale_rule_on_small_columns():
    # multiples of 2^-3 over a span of 4.5: exact at the lowest set bit
    assert CR.column_scale([3.0, 7.5, 3.125]) == (-3, 24, 1)
    # a span of more than 2^28 lowest bits: 4.5 / 2^L < 2^28 first at L = -25 (4.5 2^25 = 150994944 < 2^28 <= 4.5 2^26); rounded
    L, x0, exact = CR.column_scale([3.0, 3.0 + 2.0 ** -40, 7.5])
    assert (L, x0, exact) == (-25, 3 << 25, 0)
    assert CR.column_scale([0.0, 0.0]) == (0, 0, 1) and CR.column_scale([-2.5]) == (-1, -5, 1)
    # the width is the DIFFERENCE of the rounded ends: 0 .. 2^28 - 1 fits at L = 0, 0 .. 2^28 does not
    assert CR.column_scale([0.0, float(M28)]) == (0, 0, 1) and CR.column_scale([0.0, float(M28 + 1)])[0] == 28
    assert CR.column_scale([1.0, float(M28 + 1)]) == (0, 1, 1)


@pytest.mark.parametrize("key", KEYS)
def test_restated_cov_and_corr_of_the_golden_rows_are_numpys(G, key):
    """cov within the summation bound of numpy.cov's two passes, corr within the bound that follows from it.

    numpy.cov(V.T, ddof=0), values |v| <= M, n rows, u = 2^-53: pass 1 forms the mean with at most n roundings, |m^ - m| <= n u M, and
    the centred values x~ = fl(x - m^), |x~ - (x - m)| <= (n + 2) u M, |x - m| <= 2 M.  Pass 2 is a dot product of n terms and a
    division: (1 / n) sum x~ y~ carries the error of the factors, 2 (2 M) (n + 2) u M, and at most n + 2 roundings on terms below
    4 M^2.  Together |cov^ - cov| <= 8 (n + 2) u M^2: c = 8.
    Where a column is not exact the restatement's values are those rounded to multiples of 2^L, each within q = 2^(L - 1) of the
    row's; with R the column's range (|x - m| <= R) that moves cov_ij by at most q_i R_j + q_j R_i + q_i q_j.
    corr = c_ij / (s_i s_j): with c_ij off by e_ij and the variances by the fractions a = e_ii / c_ii, b = e_jj / c_jj <= 1 / 8,
    |corr^ - corr| <= (e_ij / (s_i s_j) + (a + b) / 2) (1 + 1 / 4) + 4 u (numpy.corrcoef's own square root and two divisions)."""
    V = G[key + "_vsi"]
    n, P = V.shape
    I = CR.integers(V)
    assert all(I["exact"]) == (key != "f64") and (key != "f64" or not any(I["exact"]))
    mean, cov, N = CR.finish(I["n"], I["L"], I["x0"], I["s"], I["raw"])
    # the integers stand for the rounded values: S_ij is sum Y_i Y_j
    Y = I["Y"].astype(object)
    for i, j in ((0, 0), (3, 77), (200, 200)):
        r = I["raw"][CR.pairs(P).index((i, j))]
        assert (r[0] << 28) + (r[1] << 14) + r[2] == int((Y[:, i] * Y[:, j]).sum())
    if key != "f64":                                                     # ... and where exact, for the rows themselves
        for j in (0, 100):
            m, var = CR.R.exact_mean_std(V[:, j])
            assert mean[j] == m and cov[j][j] == var
    M = np.abs(V).max()
    q = np.array([0.0 if e else 2.0 ** (L - 1) for e, L in zip(I["exact"], I["L"])])
    R = V.max(0) - V.min(0)
    e = 8 * (n + 2) * U * M * M + q[:, None] * R[None, :] + q[None, :] * R[:, None] + q[:, None] * q[None, :]
    c = np.array([[float(x) for x in row] for row in cov])
    got = np.cov(V.T, ddof=0)
    print("cov: largest difference %.3e, smallest bound %.3e" % (np.abs(got - c).max(), e.min()))
    assert np.all(np.abs(got - c) <= e)
    assert np.all(np.abs(np.mean(V, axis=0) - np.array([float(x) for x in mean])) <= (n + 2) * U * M + q)
    sd = np.sqrt(np.diagonal(c))
    a = np.diagonal(e) / np.diagonal(c)
    assert np.all(a <= 1 / 8.)                                           # (every golden column varies: the bound holds for every pair)
    ec = (e / np.outer(sd, sd) + (a[:, None] + a[None, :]) / 2) * 1.25 + 4 * U
    dc = np.abs(np.corrcoef(V.T) - CR.corr_float(N))
    print("corr: largest difference %.3e, smallest bound %.3e" % (dc.max(), ec.min()))
    assert np.all(dc <= ec)


# ---- bh_posterior_cov_finish ------------------------------------------------------------------------------------------------

def lib():
    from bayhunter_amd import engine as E
    return E, E.load_library()


def ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def from_patterns(patterns, counts):
    """(n, s, raw) of a table that holds row patterns[k] (integers Y, [K][P]) counts[k] times, in Python integers"""
    P = len(patterns[0])
    n = sum(counts)
    mask = (1 << CR.LIMB) - 1
    s = [sum(c * p[i] for p, c in zip(patterns, counts)) for i in range(P)]
    raw = []
    for i, j in CR.pairs(P):
        r = [0, 0, 0]
        for p, c in zip(patterns, counts):
            hi, li, hj, lj = p[i] >> CR.LIMB, p[i] & mask, p[j] >> CR.LIMB, p[j] & mask
            r[0] += c * hi * hj
            r[1] += c * (hi * lj + li * hj)
            r[2] += c * li * lj
        raw.append(r)
    return n, s, raw


def call_finish(sites, P, n_override=None):
    """bh_posterior_cov_finish on a list of sites (n, L, x0, s, raw): (rc, mean [S, P], cov, corr [S, P, P])"""
    E, L = lib()
    S = len(sites)
    n = np.array([t[0] for t in sites] if n_override is None else n_override, np.int64)
    Ls = np.array([t[1] for t in sites], np.int32).reshape(S, P)
    x0 = np.array([t[2] for t in sites], np.int64).reshape(S, P)
    s = np.array([t[3] for t in sites], np.uint64).reshape(S, P)
    raw = np.array([t[4] for t in sites], np.uint64).reshape(S, P * (P + 1) // 2, 3)
    mean, cov, corr = (np.full(sh, FILL, np.uint64).view(np.float64) for sh in ((S, P), (S, P, P), (S, P, P)))
    rc = L.bh_posterior_cov_finish(S, P, ptr(n), ptr(Ls), ptr(x0), ptr(s), ptr(raw), ptr(mean), ptr(cov), ptr(corr))
    return rc, mean, cov, corr


def finish_ok(sites, P):
    rc, mean, cov, corr = call_finish(sites, P)
    assert rc == 0
    for t, (n, L, x0, s, raw) in enumerate(sites):
        bad = CR.check_finished(mean[t], cov[t], corr[t], n, L, x0, s, raw)
        assert not bad, (t, bad[:5])
    return mean, cov, corr


BIG = (1 << 24) - 1


def test_finish_on_integers_that_stress_it():
    """columns: 0 alternates 0 / 2^28 - 1, 1 is constant at 2^28 - 1, 2 is the mirror image of 0, 3 equals 0, 4 is 2^28 - 1 but for
    one row (n S and s^2 cancel to all but a few of 104 bits)"""
    rows = [[0, M28, M28, 0, M28], [M28, M28, 0, M28, M28], [0, M28, M28, 0, M28 - 1]]
    L = [-22, 5, -22, -22, -60]
    x0 = [1 << 52, -(1 << 40), 12345, 1 << 52, 7]
    sites = []
    for counts in ((BIG // 2, BIG // 2, 1), (1, 0, 0), (3, 2, 1), (0, 1, 1)):
        n, s, raw = from_patterns(rows, counts)
        sites.append((n, L, x0, s, raw))
    sites.append((0, L, x0, [0] * 5, [[0, 0, 0]] * 15))
    assert sites[0][0] == BIG
    N = CR.numerators(*[sites[0][k] for k in (0, 3, 4)])
    # the largest variance there is (2^102), and n S = s^2 = n^2 (2^28 - 1)^2 of 104 bits cancelling to 0 and to n - 1
    assert N[0][0].bit_length() == 102 and (sites[0][3][1] ** 2).bit_length() == 104 and N[1][1] == 0 and N[4][4] == BIG - 1
    mean, cov, corr = finish_ok(sites, 5)
    c = corr[0]
    assert np.isnan(c[1]).all() and np.isnan(c[:, 1]).all() and np.all(cov[0][1] == 0) and np.all(cov[0][:, 1] == 0)
    assert c[0, 0] == c[2, 2] == c[4, 4] == 1.0
    assert abs(c[0, 3] - 1.0) <= 2.0 ** -52 and c[0, 3] <= 1.0 and abs(c[0, 2] + 1.0) <= 2.0 ** -52 and c[0, 2] >= -1.0
    assert mean[0][1] == float((M28 - (1 << 40)) * 32)
    assert np.isnan(corr[1]).all() and np.all(cov[1] == 0) and mean[1][0] == float(1 << 30)  # n = 1: (0 + 2^52) 2^-22
    assert np.isnan(mean[4]).all() and np.isnan(cov[4]).all() and np.isnan(corr[4]).all()    # n = 0


def test_finish_on_random_small_tables():
    rs = np.random.RandomState(5)
    sites = []
    P = 6
    for n in (2, 3, 5, 100, 1000):
        Y = rs.randint(0, 1 << 28, (n, P)).astype(np.int64)
        Y[:, 2] = Y[:, 0]
        Y[:, 3] = M28 - Y[:, 0]
        Y[:, 4] = Y[:, 1] // 1000 + (Y[:, 0] >> 20)
        n_, s, raw = from_patterns([[int(v) for v in row] for row in Y], [1] * n)
        sites.append((n, [int(v) for v in rs.randint(-40, 10, P)], [int(v) for v in rs.randint(-(1 << 50), 1 << 50, P)], s, raw))
    finish_ok(sites, P)


def test_finish_refuses_and_writes_nothing():
    E, L = lib()
    n, s, raw = from_patterns([[1, 2], [3, 5]], [2, 2])
    site = (n, [0, 0], [0, 0], s, raw)

    def untouched(res, code):
        rc, mean, cov, corr = res
        assert rc == code
        for a in (mean, cov, corr):
            assert np.all(a.view(np.uint64) == FILL)

    untouched(call_finish([site], 2, n_override=[1 << 24]), E.BH_EUNSUPPORTED)
    untouched(call_finish([site], 2, n_override=[-1]), E.BH_EINVAL)
    one = np.zeros(8, np.int64)
    buf = np.full(4, FILL, np.uint64)
    for S, P in ((0, 2), (1, 0), (1, 257)):
        assert L.bh_posterior_cov_finish(S, P, ptr(one), ptr(one), ptr(one), ptr(one), ptr(one), ptr(buf), None, None) == E.BH_EINVAL
    assert L.bh_posterior_cov_finish(1, 2, None, ptr(one), ptr(one), ptr(one), ptr(one), ptr(buf), None, None) == E.BH_EINVAL
    assert np.all(buf == FILL)
    rc, mean, cov, corr = call_finish([site], 2)                         # ... and the call they refuse; outputs may be NULL
    assert rc == 0 and mean[0, 0] == 2.0 and cov[0, 0, 0] == 1.0 and corr[0, 0, 1] == 1.0
    assert L.bh_posterior_cov_finish(1, 2, ptr(np.array([4], np.int64)), ptr(np.zeros(2, np.int32)), ptr(np.zeros(2, np.int64)),
                                     ptr(np.array(s, np.uint64)), ptr(np.array(raw, np.uint64)), None, None, None) == 0


def test_header_declares_what_the_library_exports():
    import os
    import re
    E, L = lib()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(here, "include", "bh_engine_posterior_cov.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(bh_[a-z_0-9]+)\s*\(", txt))) == sorted(E.POSTERIOR_COV_SYMBOLS)
    assert all(hasattr(L, name) for name in E.POSTERIOR_COV_SYMBOLS) and L.bh_abi_version() == 10
    assert int(re.search(r"#define BH_COV_MAXCOLS (\d+)", txt).group(1)) == E.COV_MAXCOLS
    assert int(re.search(r"#define BH_COV_LIMB_BITS (\d+)", txt).group(1)) == E.COV_LIMB_BITS == CR.LIMB
