"""Extended-precision reference of the likelihood (Targets.py:99-173, :322-347) with an a priori error bound.

Not a conftest: a plain module the likelihood tests import, like philox_ref.py.

What it computes
----------------
For B models of one target: the residuals d = ymod - yobs in float64, exactly as the kernels form them; everything after that
in np.longdouble (u_ld = 2^-64 on x86-64):

    Q      = d^T M d                        the law's quadratic form with M unscaled by sigma^2:
             nocorr   M = I
             scaled   M = diag(1 / s),  s = yerr / min(yerr)            (not squared, as Targets.py:117-129)
             exp      M = get_corr_inv(r): diagonal 1 + r^2 (1 at both ends), off-diagonals -r (Targets.py:131-137),
                      applied as the matrix's nonzeros (M d, then d . (M d)) -- not the closed form the kernels use
             gauss    M = R^-1 as given (host pinv)
    phi    = Q / (sigma^2 den),             den = 1 - r^2 for exp (formed as (1 - r)(1 + r), exact to u_ld), else 1
    X      = log prod(s)  |  (n-1) log(1 - r^2)  |  logdet_r  |  0
    logL   = -1/2 (n ln 2pi + 2n ln sigma + X) - phi / 2
    rms    = sqrt(sum d^2 / n)

The scaled law's X is what the reference's `np.log(np.product(scaled_err))` gives: if the float64 product overflows, X = inf
and logL = -inf.  For the Gauss law with B n^2 above LD_WORK, Q is formed in extended precision only on the rows of
sample_rows() (the first and last, both sides of every multiple of 64 -- so of 128 too -- and a few random ones); the other
rows take a float64 BLAS d @ R^-1, and their bound carries that reference's own error (below).

The bound
---------
Let u = 2^-53 and S = sum_ij |d_i| |M_ij| |d_j|, the sum of the absolute values of the terms of Q.  For the exponential law the
device evaluates the closed form (1+r^2) sum d^2 - r^2 (d_0^2 + d_{n-1}^2) - 2r sum d_i d_{i+1}, whose absolute terms add up
to S_exp = (1+r^2) sum d^2 + r^2 (d_0^2 + d_{n-1}^2) + 2|r| sum |d_i d_{i+1}| (at most 3 x the tridiagonal's own S); that is
the S used for it.

1.  Quadratic form.  Every product d_i M_ij d_j reaches the device's Q through at most m(n) = n + ceil(n/16) + 16 roundings:
    the K sum of the contraction or of the in-kernel mat-vec (<= n), the product with d_j, the epilogue's four-column sum and
    shuffles, the slab sums (<= 2 ceil(n/128) x 4 <= n/16 + 8), the block reduction; the closed forms' sums are shallower.
    The closed form adds its three scaled sums with <= 6 roundings more.  So |Q^ - Q| <= (m + 6) u S (to first order).
2.  Scaling.  sigma^2 and the division: <= 4 u |phi|.  For the exponential law r^2 is rounded (relative u) before 1 - r^2 is
    formed, so den carries a relative error <= u (r^2 / (1 - r^2) + 1): the magnification r^2/(1-r^2) of the issue near
    |r| = 1.  Together:  |phi^ - phi| <= [(m + 6) u S / (sigma^2 den)] + u (4 + r^2/(1-r^2)) |phi|.
3.  Constant part.  n log(2pi) (2pi rounded, log, product) and 2n log(sigma) (log of the device's libm: <= 2 ulp, product)
    and their sum: <= 6 u (n ln 2pi + 2n |ln sigma| + |X|).  X itself: exponential law (n-1) [u (r^2/(1-r^2) + 1) + 3 u
    |log(1-r^2)|] (the rounded 1 - r^2 through the log, the log's own rounding, the product); scaled law 2n u + 2u |X| (n
    quotients and n - 1 products on the host, then its log); Gauss 0 (logdet_r is an input).  The part is half of that.
4.  The final part - phi/2 and the sum over targets: u (|part| + |phi|/2) per target and nt u sum (|part| + |phi|/2) for
    the joint sum (JointTarget.evaluate adds the targets one after the other).
RMS misfit: sum d^2 has all-positive terms, so its error is <= m u sum d^2; the quotient by n and the square root add 2 ulp:
|rms^ - rms| <= (m/2 + 3) u rms.  The joint misfit adds nt u sum rms to the sum of the targets' bounds.

The reference's own error is added to the bound: the same derivation with u_ld in place of u, with (2n + 2) S for Q (its
sums are plain sums of n), with no magnification of 1 - r^2 (formed exactly to u_ld); on the float64 BLAS rows of the Gauss
law Q carries (2n + 2) u S instead.  `bound` is device + reference; `ref_bound` is the reference's alone.

Tolerances are FACTOR x bound (FACTOR <= 8), never fitted to what a GPU returns.
"""
import numpy as np

LAW_NOCORR, LAW_SCALED, LAW_EXP, LAW_GAUSS = 0, 1, 2, 3
LD = np.longdouble
U = 2.0 ** -53
U_LD = float(np.finfo(LD).eps) / 2.0
LN2PI = np.log(8 * np.arctan(LD(1)))      # ln(2 pi) in extended precision
LD_WORK = 1 << 24                        # Gauss law: B n^2 up to this in extended precision on every row
FACTOR = 4.0                             # tolerance = FACTOR x bound


def depth(n):
    """m(n) of the docstring: the most roundings a product of the quadratic form passes through on the device."""
    return n + -(-n // 16) + 16


def sample_rows(B, nrand=8, seed=0):
    """Rows of a batch on which the Gauss law's extended-precision quadratic form is taken: the first and the last, both sides
    of every multiple of 64 (and so of 128), and `nrand` seeded random ones."""
    rows = {0, B - 1}
    for m in range(64, B + 1, 64):
        rows.update((m - 1, m))
    rows.update(np.random.RandomState(seed).randint(0, B, size=min(nrand, B)).tolist())
    return np.array(sorted(r for r in rows if 0 <= r < B), dtype=np.int64)


class TargetRef(object):
    """logL, rms: [B] longdouble; bound, ref_bound, rms_bound: [B] float64; absterm: [B] |part| + |phi|/2 (float64)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _row(a, B):
    return np.broadcast_to(np.asarray(a, dtype=np.float64), (B,))


def target_ref(law, ymod, yobs, corr, sigma, yerr=None, rinv=None, logdet_r=0.0, ld_rows=None):
    """One target, B models: ymod [B, n]; corr, sigma scalars or [B]."""
    ymod = np.atleast_2d(np.asarray(ymod, dtype=np.float64))
    B, n = ymod.shape
    d = ymod - np.asarray(yobs, dtype=np.float64)          # float64, as the kernels form it
    dl = d.astype(LD)
    r64, sg = _row(corr, B), _row(sigma, B)
    s2 = sg.astype(LD) ** 2
    s0 = np.sum(dl * dl, axis=1)
    den = np.ones(B, dtype=LD)
    X = np.zeros(B, dtype=LD)
    mag = np.zeros(B)                                      # r^2 / (1 - r^2)
    errX, errX_ld = np.zeros(B), np.zeros(B)
    qref_u = np.full(B, U_LD)                              # unit roundoff of the reference's Q, per row
    if law == LAW_NOCORR:
        Q = s0
        S = s0.astype(np.float64)
    elif law == LAW_SCALED:
        ye = np.asarray(yerr, dtype=np.float64)
        se = ye.astype(LD) / LD(ye.min())
        Q = np.sum(dl * dl / se, axis=1)
        S = Q.astype(np.float64)
        with np.errstate(over="ignore"):
            overflow = not np.isfinite(np.prod(ye / ye.min()))   # the reference's float64 np.product
        xs = LD(np.inf) if overflow else np.log(np.prod(se))
        X[:] = xs
        errX[:] = 2 * n * U + 2 * U * float(xs)
        errX_ld[:] = 2 * n * U_LD + 2 * U_LD * float(xs)
    elif law == LAW_EXP:
        r = r64.astype(LD)
        diag = np.ones((B, n), dtype=LD) + (r * r)[:, None]
        diag[:, 0] = diag[:, -1] = 1                       # get_corr_inv: d[0] = d[-1] = 1
        v = diag * dl                                      # (M d), the tridiagonal's nonzeros
        v[:, :-1] += -r[:, None] * dl[:, 1:]
        v[:, 1:] += -r[:, None] * dl[:, :-1]
        Q = np.sum(v * dl, axis=1)
        den = (1 - r) * (1 + r)
        d64 = np.abs(d)
        edge = d64[:, 0] ** 2 + (d64[:, -1] ** 2 if n > 1 else 0.0)
        cross = np.sum(d64[:, :-1] * d64[:, 1:], axis=1)
        S = (1 + r64 ** 2) * np.sum(d64 * d64, axis=1) + r64 ** 2 * edge + 2 * np.abs(r64) * cross
        X = (n - 1) * np.log(den)
        mag = (r64 ** 2 / den.astype(np.float64))
        lg = np.abs(X.astype(np.float64)) / max(n - 1, 1)
        errX = (n - 1) * (U * (mag + 1) + 3 * U * lg)
        errX_ld = (n - 1) * (U_LD + 3 * U_LD * lg)
    elif law == LAW_GAUSS:
        M = np.ascontiguousarray(rinv, dtype=np.float64)
        S = np.einsum("bi,bi->b", np.abs(d) @ np.abs(M), np.abs(d))
        Q = np.einsum("bi,bi->b", d @ M, d).astype(LD)     # float64 BLAS on every row ...
        qref_u[:] = U
        if ld_rows is None:
            ld_rows = np.arange(B) if B * n * n <= LD_WORK else sample_rows(B)
        ML = M.astype(LD)
        for b in ld_rows:                                  # ... extended precision on the sampled ones
            Q[b] = np.dot(np.dot(dl[b], ML), dl[b])
            qref_u[b] = U_LD
        X[:] = LD(logdet_r)
    else:
        raise ValueError("unknown law %r" % law)
    phi = Q / (s2 * den)
    const = n * LN2PI + 2 * n * np.log(sg.astype(LD)) + X
    part = -const / 2
    logL = part - phi / 2
    sden = (sg ** 2) * den.astype(np.float64)
    aphi = np.abs(phi.astype(np.float64))
    abspart = n * float(LN2PI) + 2 * n * np.abs(np.log(sg)) + np.abs(X.astype(np.float64))
    m = depth(n)
    with np.errstate(invalid="ignore"):
        dev = (0.5 * ((m + 6) * U * S / sden + U * (4 + mag) * aphi)
               + 0.5 * (6 * U * abspart + errX)
               + U * (np.abs(part.astype(np.float64)) + aphi / 2))
        ref = (0.5 * ((2 * n + 2) * qref_u * S / sden + 4 * U_LD * aphi)
               + 0.5 * (6 * U_LD * abspart + errX_ld))
    rms = np.sqrt(s0 / n)
    rms64 = rms.astype(np.float64)
    return TargetRef(logL=logL, rms=rms, bound=dev + ref, ref_bound=ref,
                     rms_bound=(m / 2.0 + 3) * U * rms64 + (n + 3) * U_LD * rms64,
                     absterm=np.abs(part.astype(np.float64)) + aphi / 2)


def joint_ref(descs, ymod, noise, ld_rows=None):
    """JointTarget.evaluate's logL and misfits of B models over the engine's target descriptors (the dicts given to
    Engine.set_targets: law, n, yobs and yerr / rinv / logdet_r); ymod [B, sum n], noise [B, 2 nt].
    Returns (logL [B] longdouble, misfits [B, nt+1] longdouble, bound [B], misfit_bound [B, nt+1])."""
    ymod = np.atleast_2d(np.asarray(ymod, dtype=np.float64))
    noise = np.atleast_2d(np.asarray(noise, dtype=np.float64))
    B, nt = ymod.shape[0], len(descs)
    logL = np.zeros(B, dtype=LD)
    misf = np.zeros((B, nt + 1), dtype=LD)
    bound = np.zeros(B)
    mb = np.zeros((B, nt + 1))
    absterms = np.zeros(B)
    off = 0
    for t, dsc in enumerate(descs):
        n = int(dsc["n"])
        T = target_ref(int(dsc["law"]), ymod[:, off:off + n], dsc["yobs"], noise[:, 2 * t], noise[:, 2 * t + 1],
                       yerr=dsc.get("yerr"), rinv=dsc.get("rinv"), logdet_r=dsc.get("logdet_r", 0.0), ld_rows=ld_rows)
        logL += T.logL
        bound += T.bound
        absterms += T.absterm
        misf[:, t] = T.rms
        mb[:, t] = T.rms_bound
        off += n
    misf[:, nt] = np.sum(misf[:, :nt], axis=1)
    mb[:, nt] = np.sum(mb[:, :nt], axis=1) + nt * U * misf[:, nt].astype(np.float64)
    bound += nt * U * absterms
    return logL, misf, bound, mb


def assert_within(got, want, bound, what="", factor=FACTOR):
    """|got - want| <= factor x bound, elementwise; an infinite `want` must be returned exactly."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=LD)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), got.shape)
    inf = ~np.isfinite(want)
    assert np.array_equal(got[inf], want[inf].astype(np.float64)), "%s: non-finite reference values not returned" % what
    diff = np.abs(got[~inf].astype(LD) - want[~inf]).astype(np.float64)
    tol = factor * bound[~inf]
    bad = ~(diff <= tol)
    if np.any(bad):
        i = np.flatnonzero(bad)[0]
        idx = np.unravel_index(np.flatnonzero(~inf)[i], got.shape)
        raise AssertionError("%s: %d of %d beyond %g x the bound; first at %s: got %r, reference %r, |diff| %.3e, bound %.3e"
                             % (what, int(bad.sum()), bad.size, factor, idx, got[idx], float(want[idx]), diff[i], bound[~inf][i]))
