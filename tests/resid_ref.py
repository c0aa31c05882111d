"""A plain numpy / Python restatement of include/bh_engine_posterior_resid.h: the residual columns of one (row, slot), with the
strands and the butterfly of the header's sums written out, and its masking rules.  Every operation is one IEEE float64 operation on
Python floats / numpy float64 scalars, so the results are the header's bits (tests/test_resid_ref.py holds the sums to exact rational
arithmetic; tests/test_gpu_posterior_resid.py holds the kernel to this file)."""
import math

import numpy as np

FIXED = 5                      # BH_RESID_FIXED
MAXLAG = 32                    # BH_RESID_MAXLAG
NAMES = ("bias", "rms", "sigma_ratio", "corr", "corr_excess")


def strand_sum(terms):
    """S(x): 64 strands, strand j takes the i = j (mod 64) one after the other from +0.0; then s_j = s_j + s_{j xor w} for
    w = 32, 16, 8, 4, 2, 1, every strand at once; the sum is s_0"""
    s = [0.0] * 64
    for i, x in enumerate(terms):
        s[i % 64] = s[i % 64] + float(x)
    for w in (32, 16, 8, 4, 2, 1):
        s = [s[j] + s[j ^ w] for j in range(64)]
    return s[0]


def lag_sums(u, L):
    """A_0 .. A_L of the header: A_l = S(fl(u_i * u_{i+l})) over i < n - l"""
    u = [float(x) for x in u]
    n = len(u)
    return [strand_sum([u[i] * u[i + l] for i in range(max(n - l, 0))]) for l in range(L + 1)]


def _finite(x):
    return x if math.isfinite(x) else math.nan


def _div(a, b):
    """a / b as the device divides: IEEE, no exception"""
    return float(np.float64(a) / np.float64(b))


def columns(ymod, yobs, corr, sigma, L, g=None, err=0):
    """the FIXED + L columns of one (row, slot): ymod, yobs (and g) are the slot's n samples; corr, sigma the row's own noise
    values already widened to float64"""
    out = np.full(FIXED + L, np.nan)
    n = len(yobs)
    if err != 0 or n == 0:
        return out
    with np.errstate(all="ignore"):
        e = [float(np.float64(a) - np.float64(b)) for a, b in zip(ymod, yobs)]
        u = e if g is None else [float(np.float64(x) * np.float64(w)) for x, w in zip(e, g)]
        sb = strand_sum(e)
        se = strand_sum([float(np.float64(x) * np.float64(x)) for x in e])
        A = lag_sums(u, L)
        dn = float(n)
        corr, sigma = float(corr), float(sigma)
        acf = [math.nan] * (L + 1)
        for l in range(1, L + 1):
            if A[0] != 0.0 and l < n:
                acf[l] = _finite(_div(A[l], A[0]))
        out[0] = _finite(_div(sb, dn))
        out[1] = _finite(float(np.sqrt(np.float64(_div(se, dn)))))
        out[2] = _finite(_div(float(np.sqrt(np.float64(_div(A[0], dn)))), sigma))
        out[3] = _finite(corr)
        out[4] = _finite(float(np.float64(acf[1]) - np.float64(corr)))
        for l in range(1, L + 1):
            out[FIXED + l - 1] = acf[l]
    return out


def column_blocks(ncol):
    """every slot's first column in the synthetics: a slot's block is as wide as its largest count over the sites"""
    cap = np.asarray(ncol).max(axis=0)
    return np.concatenate(([0], np.cumsum(cap))).astype(int)


def resid_set(ymod, err, site, ncol, yobs, noise, L, g=None):
    """the RESID set [N, nt * (FIXED + L)] of N rows: ymod [N, ldy], err [N], site [N], ncol [S, nt], yobs / g [S, ldy],
    noise [N, >= 2 nt] (float32 or float64: widened)"""
    ncol = np.asarray(ncol)
    nt = ncol.shape[1]
    off = column_blocks(ncol)
    N = len(ymod)
    out = np.full((N, nt * (FIXED + L)), np.nan)
    for r in range(N):
        s = int(site[r])
        for t in range(nt):
            n = int(ncol[s, t])
            c = slice(off[t], off[t] + n)
            out[r, t * (FIXED + L):(t + 1) * (FIXED + L)] = columns(
                ymod[r, c], yobs[s, c], np.float64(noise[r, 2 * t]), np.float64(noise[r, 2 * t + 1]), L,
                None if g is None else g[s, c], int(err[r]))
    return out


def acf_model(law, r, L):
    """the autocorrelation the slot's law implies at the lags 1 .. L: r^l (exp), r^(l^2) (gauss), 0 (the uncorrelated laws)"""
    lags = np.arange(1, L + 1, dtype=np.float64)
    if law == "exp":
        return np.float64(r) ** lags
    if law == "gauss":
        return np.float64(r) ** (lags * lags)
    return np.zeros(L)
