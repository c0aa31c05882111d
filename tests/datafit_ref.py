"""A plain numpy restatement of the posterior data fits (bayhunter_amd/datafits.py, include/bh_engine_posterior_datafit.h):
the layer rule, the best fit of every chain, the masks of the DATA set, the per-site column statistics and the quantile
formula.  Written from the rules; tests/test_datafit_ref.py holds the layer rule and the best-of-chain selection bit for bit to
the reference's own outputs in tests/golden/datafit_golden.npz and the quantile formula to numpy.quantile; the GPU tests use
it as their oracle.

A row is [vs_1..vs_n, z_1..z_n, NaN...] of dtype T.  zd_j = (z_j + z_{j+1}) / 2 in T; h_j = (double)zd_j - (double)zd_{j-1}
(zd_{-1} = 0), h_{n-1} = 0; vp_j = vs_j * (T)vpvs in T, from the first layer with vs_j >= (T)mantle_vs downward vs_j *
(T)mantle_vpvs; rho_j = vp_j * (T)0.32 + (T)0.77 in T, operation by operation.
"""
import math

import numpy as np

from moho_ref import exact_mean_std  # noqa: F401  (the exact rationals of mean and variance)


def layers(row, vpvs, mantle=None):
    """(vp, vs, h, rho) of one row: vp, vs, rho in the row's dtype, h float64"""
    row = np.asarray(row)
    T = row.dtype.type
    vals = row[~np.isnan(row)]
    n = vals.size // 2
    vs, z = vals[:n], vals[n:2 * n]
    h = np.zeros(n, np.float64)
    prev = np.float64(0.0)
    for j in range(n - 1):
        zd = T((z[j] + z[j + 1]) / T(2))
        h[j] = np.float64(zd) - prev
        prev = np.float64(zd)
    k = T(vpvs)
    vp = np.zeros(n, row.dtype)
    rho = np.zeros(n, row.dtype)
    deep = False
    for j in range(n):
        if mantle is not None and mantle[0] > 0 and vs[j] >= T(mantle[0]):
            deep = True
        vp[j] = T(vs[j] * (T(mantle[1]) if deep else k))
        rho[j] = T(T(vp[j] * T(0.32)) + T(0.77))
    return vp, vs.copy(), h, rho


def layer_batch(rows, vpvs, mantle=None, ML=None):
    """(nlay int32 [B], h, vp, vs, rho float64 [ML, B]) of many rows, layer-major as the engine takes them; zeros beyond n.
    mantle: None, one pair, or one pair / None per row."""
    rows = np.asarray(rows)
    B = len(rows)
    ML = rows.shape[1] // 2 if ML is None else ML
    nlay = np.zeros(B, np.int32)
    out = [np.zeros((ML, B)) for _ in range(4)]
    per_row = mantle is not None and len(mantle) == B and (mantle[0] is None or np.ndim(mantle[0]) == 1)
    for b in range(B):
        m = mantle[b] if per_row else mantle
        vp, vs, h, rho = layers(rows[b], np.asarray(vpvs).reshape(-1)[b], m)
        n = len(vs)
        nlay[b] = n
        for a, v in zip(out, (h, vp, vs, rho)):
            a[:n, b] = v.astype(np.float64)
    return (nlay,) + tuple(out)


def best_of_chains(site, chain, misfit, nsites, nchains):
    """int64 [nsites, nchains]: the input row of the first least misfit of every (site, chain) over the rows with 0 <= site <
    nsites (numpy.argmin over the pair's rows in input order), -1 where the pair has no row"""
    site, chain = np.asarray(site), np.asarray(chain)
    misfit = np.asarray(misfit, np.float64)
    out = np.full((nsites, nchains), -1, np.int64)
    for s in range(nsites):
        for c in range(nchains):
            idx = np.flatnonzero((site == s) & (chain == c))
            if idx.size:
                out[s, c] = idx[np.argmin(misfit[idx])]
    return out


def the_best(best_row, misfit):
    """the chain of a site's best of all: the first least among its chains' bests (-1: none)"""
    have = np.flatnonzero(np.asarray(best_row) >= 0)
    if not have.size:
        return -1
    return int(have[np.argmin(np.asarray(misfit, np.float64)[np.asarray(best_row)[have]])])


def column_blocks(ncol):
    """offsets [nt + 1] of the targets' column blocks: target t's block is as wide as its largest count over the sites"""
    return np.concatenate(([0], np.cumsum(np.asarray(ncol).max(axis=0)))).astype(int)


def masked(ymod, err, site, ncol):
    """the DATA set's values [B, ldy] of a forward batch: NaN where the row failed, where the column lies beyond the site's own
    count in its target, and where the site lacks the target"""
    ymod = np.array(ymod, np.float64)
    ncol = np.asarray(ncol)
    off = column_blocks(ncol)
    assert off[-1] == ymod.shape[1]
    out = np.full(ymod.shape, np.nan)
    for b in range(len(ymod)):
        if err[b] != 0:
            continue
        for t in range(ncol.shape[1]):
            n = ncol[site[b], t]
            out[b, off[t]:off[t] + n] = ymod[b, off[t]:off[t] + n]
    return out


def quantile_rank(n, p):
    """(k, g): the virtual index (n - 1) * p of numpy.quantile's method "linear" in float64, its floor and the remainder"""
    vi = np.float64(n - 1) * np.float64(p)
    k = int(math.floor(vi))
    if k >= n - 1:
        return n - 1, np.float64(0.0)
    return k, vi - np.float64(k)


def quantile(col, p):
    """numpy.quantile(col, p, method="linear") of the values of col that are not NaN, from its order statistics: a + (b - a) * g,
    or b - (b - a) * (1 - g) where g >= 0.5; NaN for an empty column.  Also returns the two order statistics."""
    v = np.sort(np.asarray(col, np.float64)[~np.isnan(col)])
    n = len(v)
    if not n:
        return np.float64(np.nan), None, None
    k, g = quantile_rank(n, p)
    a, b = v[k], v[min(k + 1, n - 1)]
    d = b - a
    return (b - d * (np.float64(1) - g) if g >= 0.5 else a + d * g), a, b


def column_summary(col, quantiles=()):
    """count, nan, min, max, median of one column over its values that are not NaN, and its quantiles"""
    col = np.asarray(col, np.float64)
    v = col[~np.isnan(col)]
    out = dict(count=len(v), nan=int(len(col) - len(v)))
    if len(v):
        out.update(min=v.min(), max=v.max(), median=np.median(v))
    else:
        out.update(min=np.nan, max=np.nan, median=np.nan)
    out["quantiles"] = np.array([quantile(col, p)[0] for p in quantiles])
    return out


def plan_is_sound(rows, ldy, max_bytes, groups):
    """what the group planner must hold: the groups are consecutive and cover every site once; none is over the budget unless
    it is a single site"""
    S = len(rows)
    if not S:
        return groups == []
    if groups[0][0] != 0 or groups[-1][1] != S:
        return False
    for (a0, a1), (b0, b1) in zip(groups[:-1], groups[1:]):
        if a1 != b0:
            return False
    for s0, s1 in groups:
        if s1 <= s0:
            return False
        if sum(rows[s0:s1]) * ldy * 8 > max_bytes and s1 - s0 > 1:
            return False
    return True
