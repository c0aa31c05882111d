"""A plain numpy restatement of the Moho rule and of the per-site statistics of scalar columns (bayhunter_amd/posterior.py,
include/bh_engine_posterior_scalars.h), written from the rules, held bit for bit to the reference's own outputs in
tests/golden/moho_golden.npz (tests/test_moho_ref.py) and used as the GPU tests' oracle.

A row is [vs_1..vs_n, z_1..z_n, NaN...].  zd_j = (z_j + z_{j+1}) / 2 in the row's dtype, h_j = (double)zd_j - (double)zd_{j-1},
ifaces_j = the sequential float64 sum of h_0..h_j.  The Moho is the smallest k in 0..n-2 with lo < ifaces_k < hi (both strict)
and (double)vs_{k+1} > mohovs; moho = ifaces_k, vslast = vs_k, vsjump = vs_{k+1} - vs_k (row dtype), vscrust = S / ifaces_k with
S = sum_{j<=k} (double)vs_j * h_j in numpy.sum's order (np_sum below).
"""
import numpy as np

import posterior_ref as R

COLUMNS = ("moho", "vslast", "vscrust", "vsjump")


def np_sum(a):
    """numpy.sum of a contiguous float64 vector of fewer than 128 terms, addition by addition: sequential below 8 terms; else
    eight strided accumulators over the whole blocks of 8, combined pairwise, the remaining terms added sequentially."""
    n = len(a)
    if n < 8:
        res = np.float64(0.0)
        for x in a:
            res = res + x
        return res
    r = [np.float64(a[i]) for i in range(8)]
    i = 8
    while i < n - (n % 8):
        for t in range(8):
            r[t] = r[t] + a[i + t]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    while i < n:
        res = res + a[i]
        i += 1
    return res


def moho_rows(models, lo, hi, mohovs):
    """float64 [Nkept, 4] (moho, vslast, vscrust, vsjump), NaN for a row without a Moho; rows of NaN only are left out."""
    models = np.asarray(models)
    T = models.dtype.type
    n_all, keep = R.split(models)
    out = []
    for row, n in zip(models[keep], n_all[keep]):
        vs, z = row[:n], row[n:2 * n]
        zd = (z[:-1] + z[1:]) / T(2)                      # row dtype
        zd64 = zd.astype(np.float64)
        h = zd64 - np.concatenate((np.zeros(1), zd64[:-1]))
        ifaces = np.zeros(n - 1)
        acc = np.float64(0.0)
        for j in range(n - 1):
            acc = h[j] if j == 0 else acc + h[j]
            ifaces[j] = acc
        k = -1
        for j in range(n - 1):
            if lo < ifaces[j] < hi and np.float64(vs[j + 1]) > mohovs:
                k = j
                break
        if k < 0:
            out.append((np.nan,) * 4)
            continue
        terms = vs[:k + 1].astype(np.float64) * h[:k + 1]
        out.append((ifaces[k], np.float64(vs[k]), np_sum(terms) / ifaces[k], np.float64(T(vs[k + 1] - vs[k]))))
    return np.array(out, dtype=np.float64).reshape(-1, 4)


def exact_mean_std(col):
    """Exact rational mean and population variance (Fractions) of the values of one column, NaN left out: what the integer
    sums of the device stand for (the same arithmetic as posterior_ref.exact_mean_std)."""
    col = np.asarray(col, np.float64)
    return R.exact_mean_std(col[~np.isnan(col)])


def nlayers(models):
    """n - 1 of every kept row (float64, as the reference's model.size / 2 - 1)"""
    n, keep = R.split(np.asarray(models))
    return (n[keep] - 1).astype(np.float64)


def median(v):
    """numpy.median, in the dtype of v: the middle value of the sorted column, or the mean of the two middle ones"""
    s = np.sort(v)
    n = len(s)
    if n % 2:
        return s[n // 2]
    with np.errstate(over="ignore"):
        return (s[n // 2 - 1] + s[n // 2]) / v.dtype.type(2)


def hist(v, edges):
    """numpy.histogram counts of v over edges (searchsorted 'right', the last edge into the last bin)"""
    v = np.asarray(v, np.float64)
    b = R.hist_bins(v, np.asarray(edges, np.float64))
    return np.bincount(b[b >= 0], minlength=len(edges) - 1)


def hist2d(x, y, xedges, yedges):
    """numpy.histogram2d counts [nx, ny]"""
    bx = R.hist_bins(np.asarray(x, np.float64), np.asarray(xedges, np.float64))
    by = R.hist_bins(np.asarray(y, np.float64), np.asarray(yedges, np.float64))
    ok = (bx >= 0) & (by >= 0)
    nx, ny = len(xedges) - 1, len(yedges) - 1
    return np.bincount(bx[ok] * ny + by[ok], minlength=nx * ny).reshape(nx, ny)


def mode2d(counts, xedges, yedges):
    """the centres of the first largest cell, x-major (numpy.unravel_index(argmax))"""
    xi, yi = np.unravel_index(np.argmax(counts), counts.shape)
    return ((xedges[:-1] + xedges[1:]) / 2.)[xi], ((yedges[:-1] + yedges[1:]) / 2.)[yi]


def moho_summary(models, lo, hi, mohovs, bins=50, rows=None):
    """What posterior_moho returns for one site, from the restated rows with numpy's own edges (rows: moho_rows of the same
    arguments, where the caller has them already)."""
    if rows is None:
        rows = moho_rows(models, lo, hi, mohovs)
    v = rows[~np.isnan(rows[:, 3])]
    out = dict(rows=len(rows), count=len(v), values=v, hist={}, hist2d={}, mode={})
    if not len(v):
        return out
    edges = [np.histogram_bin_edges(v[:, q], bins) for q in range(4)]
    for q, name in enumerate(COLUMNS):
        out[name] = dict(median=median(v[:, q]), min=v[:, q].min(), max=v[:, q].max())
        out["hist"][name] = (hist(v[:, q], edges[q]), edges[q])
    for q in (1, 2, 3):
        c = hist2d(v[:, q], v[:, 0], edges[q], edges[0])
        out["hist2d"][COLUMNS[q]] = (c, edges[q], edges[0])
        out["mode"][COLUMNS[q]] = mode2d(c, edges[q], edges[0])
    return out


def scalar_summary(v, bins=20, nlayer_edges=False):
    """What posterior_scalars returns for one column of one site: v in its own dtype, NaN = no value."""
    v = np.asarray(v)
    ok = ~np.isnan(v)
    x = v[ok]
    out = dict(count=len(x), nan=int((~ok).sum()))
    if not len(x):
        return out
    mn, mx = x.min(), x.max()
    if nlayer_edges:
        edges = np.arange(mn, mx + 2) - 0.5
    elif mn == mx:
        m = float(mn)
        edges = np.array([m - 1, m - 0.1, m + 0.1, m + 1])
    else:
        edges = np.histogram_bin_edges(x, bins)
    cnt = hist(x, edges)
    out.update(median=median(x), min=mn, max=mx, constant=bool(mn == mx), hist=(cnt, edges),
               mode=((edges[:-1] + edges[1:]) / 2.)[np.argmax(cnt)])
    return out
