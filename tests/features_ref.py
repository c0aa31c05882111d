"""A plain restatement of the structural features of a layered model (include/bh_engine_posterior_features.h,
bayhunter_amd/posterior.py: posterior_features), written from the rules: one Python loop per row, float64 scalars, the row
dtype's own subtraction for a jump, no vectorised sums.  tests/test_features_ref.py holds it to things that are not the
restatement (an integration of the step model, tests/moho_ref.py, numpy's argmin / argmax); the GPU tests use it as their oracle.

A row is [vs_1..vs_n, z_1..z_n, NaN...].  zd_j = (z_j + z_{j+1}) / 2 in the row's dtype, d_j = the sequential float64 sum of
(double)zd_j - (double)zd_{j-1} (zd_{-1} = 0), j = 0..n-2.  Layer j covers [t_j, b_j): t_0 = 0, t_j = d_{j-1}, b_j = d_j,
b_{n-1} = +inf.  For a window z0 < z1: len_j = min(b_j, z1) - max(t_j, z0), layer j is in the window where len_j > 0; interface k
is in the window where z0 < d_k < z1; jump_k = (double)(T)(vs_{k+1} - vs_k).
"""
import numpy as np

KINDS = ("vsmean", "vstime", "tts", "vsmin", "vsmax", "drop", "jump", "above", "nifaces")   # BH_FEATURE_* 0..8
NCOLS = dict(vsmean=1, vstime=1, tts=1, vsmin=2, vsmax=2, drop=2, jump=2, above=1, nifaces=1)
NAN = np.float64(np.nan)
INF = np.float64(np.inf)


def row_model(row):
    """(vs [n] in the row's dtype, d [n-1] float64) of one row; n = 0 for a row of NaN only"""
    row = np.asarray(row)
    T = row.dtype.type
    n = int((~np.isnan(row)).sum()) // 2
    vs, z = row[:n], row[n:2 * n]
    d = np.zeros(max(n - 1, 0))
    acc = np.float64(0.0)
    prev = np.float64(0.0)
    for j in range(n - 1):
        zd = np.float64(T((z[j] + z[j + 1]) / T(2)))
        h = zd - prev
        acc = h if j == 0 else acc + h
        d[j] = acc
        prev = zd
    return vs, d


def finite(v):
    return v if np.isfinite(v) else NAN


def layers(n, d, z0, z1):
    """(j, top, len_j) of the layers in the window, ascending"""
    t = np.float64(0.0)
    for j in range(n):
        b = d[j] if j < n - 1 else INF
        top = max(t, z0)
        ln = min(b, z1) - top
        if ln > 0.0:
            yield j, top, ln
        t = b


def feature(kind, vs, d, z0, z1, c):
    """the one or two float64 values of one feature of one row"""
    T = vs.dtype.type
    n = len(vs)
    z0, z1, c = np.float64(z0), np.float64(z1), np.float64(c)
    with np.errstate(all="ignore"):
        if kind in ("vsmean", "vstime", "tts"):
            s = np.float64(0.0)
            for j, _, ln in layers(n, d, z0, z1):
                s = s + (np.float64(vs[j]) * ln if kind == "vsmean" else ln / np.float64(vs[j]))
            if kind == "vsmean":
                return (finite(s / (z1 - z0)),)
            if kind == "vstime":
                return (finite((z1 - z0) / s),)
            return (finite(s),)
        if kind in ("vsmin", "vsmax"):
            best, dep = None, NAN
            for j, top, _ in layers(n, d, z0, z1):
                v = np.float64(vs[j])
                if best is None or (v > best if kind == "vsmax" else v < best):
                    best, dep = v, top
            return (NAN, NAN) if best is None else (finite(best), finite(dep))
        inside = [k for k in range(n - 1) if z0 < d[k] < z1]
        if kind in ("drop", "jump"):
            best, dep = None, NAN
            for k in inside:
                jm = np.float64(T(vs[k + 1] - vs[k]))
                if best is None or (jm > best if kind == "jump" else jm < best):
                    best, dep = jm, d[k]
            if best is None or not (best > c if kind == "jump" else best < -c):
                return (NAN, NAN)
            return (finite(dep), finite(best))
        if kind == "above":
            for k in inside:
                if np.float64(vs[k + 1]) > c:
                    return (finite(d[k]),)
            return (NAN,)
        if kind == "nifaces":
            return (np.float64(len(inside)),)
    raise ValueError("unknown kind %r" % (kind,))


def features_ref(models, kinds, par, site=None):
    """float64 [ncols][N]: the feature table of the rows (none of them NaN only).  kinds: [F] names or BH_FEATURE_* numbers; par
    [S][F][3] = (z0, z1, c) per (site, feature); site [N] (None: every row is site 0).  Columns feature after feature."""
    models = np.asarray(models)
    kinds = [k if isinstance(k, str) else KINDS[int(k)] for k in kinds]
    par = np.asarray(par, np.float64)
    N = len(models)
    site = np.zeros(N, np.int64) if site is None else np.asarray(site)
    out = np.full((sum(NCOLS[k] for k in kinds), N), np.nan)
    for r in range(N):
        vs, d = row_model(models[r])
        if not len(vs):
            raise ValueError("row %d holds no model" % r)
        q = 0
        for f, k in enumerate(kinds):
            z0, z1, c = par[site[r], f]
            for v in feature(k, vs, d, z0, z1, c):
                out[q, r] = v
                q += 1
    return out
