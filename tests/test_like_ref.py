"""The extended-precision likelihood reference (tests/like_ref.py) against the oracle's dense float64 restatement of
Targets.py and against mpmath at 40 digits.  CPU only."""
import mpmath
import numpy as np
import pytest

import like_ref as LR


def _rinv(n, corr=0.5):
    idx = np.arange(n)
    R = corr ** ((idx[:, None] - idx[None, :]).astype(float) ** 2)
    return np.linalg.pinv(R, rcond=1e-6), float(np.linalg.slogdet(R)[1])


def _case(law, n, rs):
    kw = {}
    if law == LR.LAW_SCALED:
        kw["yerr"] = rs.uniform(0.5, 2.0, n)
    if law == LR.LAW_GAUSS:
        kw["rinv"], kw["logdet_r"] = _rinv(n)
    return kw


@pytest.mark.parametrize("law", [LR.LAW_NOCORR, LR.LAW_SCALED, LR.LAW_EXP, LR.LAW_GAUSS])
@pytest.mark.parametrize("n", [2, 3, 30, 201])
def test_reference_matches_the_oracle(oracle, law, n):
    """Well-conditioned cases (r = 0.5 for the Gauss law, |r| <= 0.75): the helper and oracle.loglike_dense (the dense
    n x n C^-1 of Targets.py in float64) agree to 1e-12, and the RMS misfits to 1e-13."""
    rs = np.random.RandomState(100 * law + n)
    B = 6
    yobs = rs.normal(0, 1, n)
    ymod = yobs + rs.normal(0, 0.1, (B, n))
    corr = np.array([0.0, 0.35, -0.5, 0.75, -0.75, 0.1])
    sigma = rs.uniform(0.02, 0.2, B)
    kw = _case(law, n, rs)
    T = LR.target_ref(law, ymod, yobs, corr, sigma, **kw)
    for b in range(B):
        o = oracle.loglike_dense(law, ymod[b], yobs, corr[b], sigma[b], **kw)
        assert abs(float(T.logL[b]) - o) <= 1e-12 * abs(o), (b, float(T.logL[b]), o)
        assert abs(float(T.rms[b]) - oracle.rms(ymod[b], yobs)) <= 1e-13 * float(T.rms[b])


def _mp_loglike(law, d, corr, sigma, yerr=None, rinv=None, logdet_r=0.0):
    """Targets.py:105-173, :339-342 at 40 digits from the float64 residuals: the dense C^-1 and its quadratic form."""
    n = len(d)
    d = [mpmath.mpf(float(x)) for x in d]
    r, s = mpmath.mpf(float(corr)), mpmath.mpf(float(sigma))
    if law == LR.LAW_NOCORR:
        M = mpmath.eye(n)
        X, den = mpmath.mpf(0), mpmath.mpf(1)
    elif law == LR.LAW_SCALED:
        emin = mpmath.mpf(float(min(yerr)))
        se = [mpmath.mpf(float(e)) / emin for e in yerr]
        M = mpmath.diag([1 / v for v in se])
        X, den = mpmath.log(mpmath.fprod(se)), mpmath.mpf(1)
    elif law == LR.LAW_EXP:
        M = mpmath.zeros(n, n)
        for i in range(n):
            M[i, i] = 1 if i in (0, n - 1) else 1 + r * r
            if i + 1 < n:
                M[i, i + 1] = M[i + 1, i] = -r
        den = 1 - r * r
        X = (n - 1) * mpmath.log(den)
    else:
        M = mpmath.matrix([[mpmath.mpf(float(x)) for x in row] for row in rinv])
        X, den = mpmath.mpf(float(logdet_r)), mpmath.mpf(1)
    Q = mpmath.fsum(d[i] * M[i, j] * d[j] for i in range(n) for j in range(n))
    rms = mpmath.sqrt(mpmath.fsum(x * x for x in d) / n)
    return -(n * mpmath.log(2 * mpmath.pi) + 2 * n * mpmath.log(s) + X) / 2 - Q / (s * s * den) / 2, rms


@pytest.mark.parametrize("law", [LR.LAW_NOCORR, LR.LAW_SCALED, LR.LAW_EXP, LR.LAW_GAUSS])
@pytest.mark.parametrize("n", [1, 2, 3, 17, 40])
def test_reference_is_within_its_own_bound_of_40_digits(law, n):
    """mpmath at 40 digits on the same float64 residuals: the helper is within the bound it states for itself (ref_bound), and
    so within its full bound; r = +-0.9999 included, where 1 - r^2 = 2e-4 and a float64 1 - r^2 alone would be off by more.
    The Gauss law uses the ill-conditioned pinv of 0.92^((i-j)^2) (entries of R^-1 up to ~1e6 at n = 40)."""
    rs = np.random.RandomState(7 * n + law)
    corr = np.array([-0.9999, -0.5, 0.0, 0.35, 0.9999])
    B = corr.size
    yobs = rs.normal(0, 1, n)
    d = rs.normal(0, 1, (B, n)) * (10.0 ** rs.uniform(-3, 3, B))[:, None]
    d[1] = np.cumsum(d[1]) * 1e-3                        # a smooth row: strong cancellation in the cross terms
    ymod = yobs + d
    sigma = rs.uniform(0.01, 0.1, B)
    kw = {}
    if law == LR.LAW_SCALED:
        kw["yerr"] = 10.0 ** rs.uniform(-3, 1, n)
    if law == LR.LAW_GAUSS:
        idx = np.arange(n)
        R = 0.92 ** ((idx[:, None] - idx[None, :]).astype(float) ** 2)
        kw["rinv"], kw["logdet_r"] = np.linalg.pinv(R, rcond=1e-6), float(np.linalg.slogdet(R)[1])
    T = LR.target_ref(law, ymod, yobs, corr, sigma, **kw)
    for b in range(B):
        with mpmath.workdps(40):
            ll, rms = _mp_loglike(law, ymod[b] - yobs, corr[b], sigma[b], **kw)
            # the helper's longdouble, exactly, as its float64 part plus the remainder
            err = abs(mpmath.mpf(float(T.logL[b])) + mpmath.mpf(float(T.logL[b] - LR.LD(float(T.logL[b])))) - ll)
            e_rms = abs(mpmath.mpf(float(T.rms[b])) + mpmath.mpf(float(T.rms[b] - LR.LD(float(T.rms[b])))) - rms)
        assert err <= T.ref_bound[b] <= T.bound[b], (law, n, b, float(err), T.ref_bound[b])
        assert e_rms <= T.rms_bound[b], (law, n, b, float(e_rms), T.rms_bound[b])


def test_float64_device_arithmetic_is_within_the_bound():
    """The bound is not vacuous and not too tight: the closed form the kernels evaluate, restated in float64 with NumPy, lands
    within 1 x the bound of the extended-precision value, also at r = +-0.9999 on smooth residuals and at n = 65536; a doubled
    edge term at n = 1 or a dropped last cross term does not."""
    rs = np.random.RandomState(5)
    for n in (1, 2, 65, 1024, 65536):
        corr = np.array([-0.9999, -0.5, 0.0, 0.75, 0.99, 0.9999])
        B = corr.size
        yobs = rs.normal(0, 1, n)
        d = np.cumsum(rs.normal(0, 1, (B, n)), axis=1) * (10.0 ** rs.uniform(-3, 3, B))[:, None]
        ymod = yobs + d
        sigma = rs.uniform(0.01, 0.1, B)
        T = LR.target_ref(LR.LAW_EXP, ymod, yobs, corr, sigma)
        dd = ymod - yobs

        def closed(edge_twice=False, drop_last=False):
            s0 = np.sum(dd * dd, axis=1)
            s1 = np.sum(dd[:, :-1] * dd[:, 1:], axis=1)
            if drop_last and n > 1:
                s1 = s1 - dd[:, -2] * dd[:, -1]
            edge = dd[:, 0] ** 2 + dd[:, -1] ** 2 if (n > 1 or edge_twice) else dd[:, 0] ** 2
            r2 = corr * corr
            phi = ((1.0 + r2) * s0 - r2 * edge - 2.0 * corr * s1) / (sigma * sigma * (1.0 - r2))
            return -0.5 * (n * np.log(2 * np.pi) + 2.0 * n * np.log(sigma) + (n - 1) * np.log(1.0 - r2)) - phi / 2.0

        LR.assert_within(closed(), T.logL, T.bound, "float64 closed form, n=%d" % n, factor=1.0)
        rn0 = corr != 0                                   # (at r = 0 neither term counts)
        if n == 1:
            assert np.all(np.abs(closed(edge_twice=True) - T.logL.astype(np.float64))[rn0] > 8 * T.bound[rn0])
        if n in (2, 65):
            assert np.all(np.abs(closed(drop_last=True) - T.logL.astype(np.float64))[rn0] > 8 * T.bound[rn0])


def test_sample_rows():
    rows = LR.sample_rows(300)
    for r in (0, 63, 64, 127, 128, 191, 192, 255, 256, 299):
        assert r in rows
    assert rows.min() >= 0 and rows.max() <= 299 and np.all(np.diff(rows) > 0)
    assert list(LR.sample_rows(1)) == [0]


def test_scaled_law_overflow_is_the_references_minus_infinity():
    """np.log(np.product(yerr / yerr.min())) overflows to inf in float64 for long, wide error bars: the reference's logL is then
    -inf, and so is the helper's (its longdouble product would not overflow)."""
    rs = np.random.RandomState(3)
    n = 400
    yerr = 10.0 ** rs.uniform(-3, 1, n)
    with np.errstate(over="ignore"):
        assert np.isinf(np.prod(yerr / yerr.min()))
    yobs = rs.normal(0, 1, n)
    T = LR.target_ref(LR.LAW_SCALED, yobs + rs.normal(0, 0.1, (3, n)), yobs, 0.0, 0.05, yerr=yerr)
    assert np.all(T.logL == -np.inf) and np.all(np.isfinite(T.rms))
