"""A vectorised numpy restatement of the posterior summaries (bayhunter_amd/posterior.py, include/bh_engine_posterior.h),
written from the rules, checked against the reference's own outputs in tests/golden/posterior_golden.npz
(tests/test_posterior_ref.py) and used as the GPU tests' oracle.

Rows are [vs_1..vs_n, z_1..z_n, NaN...].  zd_j = (z_j + z_{j+1}) / 2 in the row's dtype; the step model's depths
d_j = cumsum(zd_j - zd_{j-1}) in float64; the interface depths of the 2-D plot are the same sums in the row's dtype of
the differences rounded to it.  vs at depth x = vs[#{j : d_j <= x}].
"""
from fractions import Fraction
import math

import numpy as np

NO_BIT = np.iinfo(np.int32).max   # low_bit of 0.0: it has no set bit


def split(models):
    """(n [N], keep [N]) -- n = 0 for NaN-only rows; ValueError for a row that is not a prefix of even length."""
    ok = ~np.isnan(models)
    c = ok.sum(1)
    first = np.where(ok.all(1), models.shape[1], np.argmin(ok, axis=1))
    bad = (c > 0) & ((c != first) | (c % 2 == 1))
    if bad.any():
        raise ValueError("rows %s are not a prefix of even length" % np.flatnonzero(bad)[:5])
    return c // 2, c > 0


def depths(models):
    """vs [N, ML] (row dtype, NaN padded), d [N, ML-1] float64, di [N, ML-1] row dtype (NaN beyond n-1), n [N]."""
    n, keep = split(models)
    models = models[keep]
    n = n[keep]
    N, W = models.shape
    ML = W // 2
    cols = np.arange(ML)
    vs = np.where(cols[None, :] < n[:, None], models[:, :ML], np.nan).astype(models.dtype)
    zi = np.clip(n[:, None] + cols[None, :], 0, W - 1)
    z = np.take_along_axis(models, zi, axis=1)
    z = np.where(cols[None, :] < n[:, None], z, np.nan).astype(models.dtype)
    zd = (z[:, :-1] + z[:, 1:]) / models.dtype.type(2)       # NaN beyond n-1
    zd64 = zd.astype(np.float64)
    h = np.diff(np.concatenate((np.zeros((N, 1)), zd64), axis=1), axis=1)
    d = np.cumsum(np.nan_to_num(h), axis=1)
    hi = np.nan_to_num(h).astype(models.dtype)
    di = np.cumsum(hi, axis=1, dtype=models.dtype)
    live = cols[None, :-1] < (n - 1)[:, None]
    return vs, np.where(live, d, np.nan), np.where(live, di, np.nan).astype(models.dtype), n


def interp(models, dep, chunk=2048):
    """vs of every kept row at every depth: float64 [Nkept, D]."""
    vs, d, _, _ = depths(models)
    dep = np.asarray(dep, np.float64)
    out = np.empty((len(vs), dep.size))
    for a in range(0, len(vs), chunk):
        k = (d[a:a + chunk, None, :] <= dep[None, :, None]).sum(2)
        out[a:a + chunk] = np.take_along_axis(vs[a:a + chunk].astype(np.float64), k, axis=1)
    return out


def hist_bins(v, edges):
    """numpy.histogram(dd)'s bin of every value (searchsorted 'right', the last edge into the last bin); -1 outside."""
    idx = np.searchsorted(edges, v, side="right")
    idx[v == edges[-1]] -= 1
    return np.where((idx >= 1) & (idx <= edges.size - 1), idx - 1, -1)


def hist2d(vsi, samples, vs_edges, dep_edges):
    """counts [nvs, ndep] of vsi [N, D] sampled at `samples`."""
    bv = hist_bins(vsi.ravel(), np.asarray(vs_edges, np.float64))
    bd = np.tile(hist_bins(np.asarray(samples, np.float64), np.asarray(dep_edges, np.float64)), len(vsi))
    ok = (bv >= 0) & (bd >= 0)
    nd = len(dep_edges) - 1
    return np.bincount(bv[ok] * nd + bd[ok], minlength=(len(vs_edges) - 1) * nd).reshape(len(vs_edges) - 1, nd)


def interface_hist(models, edges):
    _, _, di, _ = depths(models)
    v = di[~np.isnan(di)].astype(np.float64)
    b = hist_bins(v, np.asarray(edges, np.float64))
    return np.bincount(b[b >= 0], minlength=len(edges) - 1)


def median(vsi):
    """numpy's rule on sorted columns: the middle value, or (a + b) / 2 of the two middle values."""
    s = np.sort(vsi, axis=0)
    N = len(s)
    if N % 2:
        return s[N // 2].copy()
    return (s[N // 2 - 1] + s[N // 2]) / 2.


def mode(vsi, dep):
    """(vs_mode, dep_center, valid): the first maximum of histogram2d(vs, dep, bins=(vsbins, dep)) per depth bin."""
    vmin, vmax = vsi.min(), vsi.max()
    nb = int((vmax - vmin) / 0.025)
    dep = np.asarray(dep, np.float64)
    dc = (dep[:-1] + dep[1:]) / 2.
    if nb == 0:
        return np.full(dep.size - 1, np.nan), dc, False
    e = np.linspace(vmin, vmax, nb + 1)
    c = hist2d(vsi, dep, e, dep)
    return ((e[:-1] + e[1:]) / 2.)[np.argmax(c, axis=0)], dc, True


def exact_mean_std(col):
    """Exact rational mean and population variance of one column (Fractions)."""
    fr = [Fraction(float(v)) for v in col]
    n = len(fr)
    m = sum(fr) / n
    return m, sum((f - m) ** 2 for f in fr) / n


def low_bit(v):
    """The exponent of the lowest set bit of every float64 value (NO_BIT for +-0): v is an odd multiple of 2^low_bit."""
    m, e = np.frexp(np.asarray(v, np.float64))                    # |m| in [0.5, 1): m * 2^53 is an integer
    mi = np.ldexp(np.abs(m), 53).astype(np.int64)
    tz = np.frexp((mi & -mi).astype(np.float64))[1] - 1           # trailing zeros (a power of two converts exactly)
    return np.where(mi == 0, NO_BIT, e.astype(np.int64) - 53 + tz)


def scale_rule(vsi):
    """The fixed-point rule of include/bh_engine_posterior.h for every column of vsi [N, D], N >= 1: (scale, x0, exact), lists of
    Python ints.  scale = the lowest set bit of the column, raised to ea - 62 where max|v| < 2^ea would not stay below 2^62 (exact
    = 0 then); a column of zeros has scale 0; x0 = rint(min * 2^-scale)."""
    vsi = np.asarray(vsi, np.float64)
    low = low_bit(vsi).min(0)
    vmn = vsi.min(0)
    amax = np.maximum(np.abs(vmn), np.abs(vsi.max(0)))
    scale, x0, exact = [], [], []
    for j in range(vsi.shape[1]):
        L, ex = 0, 1
        if amax[j] > 0:
            ea = math.frexp(amax[j])[1]
            L, ex = max(int(low[j]), ea - 62), int(low[j] >= ea - 62)
        scale.append(L)
        exact.append(ex)
        x0.append(int(Fraction(float(vmn[j])) * Fraction(2) ** -L) if ex else int(np.rint(np.ldexp(vmn[j], -L))))
    return scale, x0, exact


def _colsum(u):
    """Exact column sums of a uint64 array (fewer than 2^32 rows) as Python ints."""
    lo = (u & np.uint64(0xffffffff)).sum(0, dtype=np.uint64)
    hi = (u >> np.uint64(32)).sum(0, dtype=np.uint64)
    return [int(a) + (int(b) << 32) for a, b in zip(lo, hi)]


def int_sums(vsi, scale, x0):
    """Per column (sum(Y), sum(Y * Y)) as Python ints, Y = rint(v * 2^-scale) - x0 (an integer in [0, 2^63))."""
    vsi = np.asarray(vsi, np.float64)
    X = np.rint(np.ldexp(vsi, -np.asarray(scale, np.int32)[None, :])).astype(np.int64)   # |X| < 2^62: exact in int64
    Y = X - np.asarray(x0, np.int64)[None, :]
    assert (Y >= 0).all()
    Y = Y.astype(np.uint64)
    a, b = Y & np.uint64(0xffffffff), Y >> np.uint64(32)          # Y = a + b 2^32: a^2, a b and b^2 fit 64 bits
    s1 = _colsum(Y)
    aa, ab, bb = _colsum(a * a), _colsum(a * b), _colsum(b * b)
    return s1, [p + (q << 33) + (r << 64) for p, q, r in zip(aa, ab, bb)]


def exact_mean(n, s1, scale, x0):
    """The exact mean of a column from sum(Y): a Fraction."""
    return Fraction(s1 + n * x0, n) * Fraction(2) ** scale


def exact_std(n, s1, s2, scale, bits=100):
    """The population std of a column from its integer sums, as a Fraction carried to `bits` bits: floor(sqrt(V) 2^k) / 2^k
    with V = n sum(Y^2) - sum(Y)^2 = n^2 var 2^(-2 scale), below the exact value by less than 2^-bits of it."""
    V = n * s2 - s1 * s1
    assert V >= 0
    k = max(0, bits - V.bit_length() // 2 + 1)
    return Fraction(math.isqrt(V << (2 * k)), n << k) * Fraction(2) ** scale


def singlemodels(models, dep):
    vsi = interp(models, dep)
    vm, dc, ok = mode(vsi, dep)
    return dict(vsi=vsi, median=median(vsi), min=vsi.min(0), max=vsi.max(0), mode=vm, dep_center=dc, mode_valid=ok)
