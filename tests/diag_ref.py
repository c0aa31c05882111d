"""A plain restatement of the chain diagnostics (include/bh_engine_chain_diag.h, bayhunter_amd/diagnostics.py) that imports nothing
of the package: the sums of a series with math.fsum as the exact sum of their float64 terms, and the formulas of split R-hat and
of Stan's effective sample size as loops over Python floats.

Every sum comes with the bound of floating-point summation in any order: a sum s of n float64 terms t_i formed by n - 1 rounded
additions obeys  |s - sum t_i| <= (n - 1) u / (1 - (n - 1) u) * sum |t_i|  <=  n * 2^-53 * sum |t_i|   (u = 2^-53, n < 9e7).
"""
import math

import numpy as np

U = 2.0 ** -53


def _sum(terms):
    """(the exact sum rounded once, its bound) of float64 terms"""
    terms = np.asarray(terms, dtype=np.float64)
    if not terms.size:
        return 0.0, 0.0
    return math.fsum(terms), terms.size * U * math.fsum(np.abs(terms))


def halves(T):
    h = T // 2
    return h, slice(0, h), slice(T - h, T)


def pass1(x):
    """x [T] (any float dtype): x0, d [T], and (value, bound) of S1, S1a, S1b"""
    x = np.asarray(x)
    T = x.shape[0]
    x0 = float(x[0])
    d = x.astype(np.float64) - x0
    h, a, b = halves(T)
    return dict(x0=x0, d=d, s1=_sum(d), s1a=_sum(d[a]), s1b=_sum(d[b]))


def means(T, s1, s1a, s1b):
    """m, ma, mb as the engine forms them from the sums it returned (float64 divisions)"""
    h = T // 2
    return s1 / float(T), (s1a / float(h) if h else 0.0), (s1b / float(h) if h else 0.0)


def pass2(d, m, ma, mb, L):
    """(value, bound) of M2a, M2b and the list of those of P_k, k = 0..L, from d [T] and the means"""
    d = np.asarray(d, dtype=np.float64)
    T = d.shape[0]
    h, a, b = halves(T)
    ua, ub = d[a] - ma, d[b] - mb
    e = d - m
    p = [_sum(e[:T - k] * e[k:]) if k < T else (0.0, 0.0) for k in range(L + 1)]
    return dict(m2a=_sum(ua * ua), m2b=_sum(ub * ub), p=p)


def tables(x, L):
    """the table of bayhunter_amd.diagnostics.chain_series_stats for x [T][C][Q], every sum exact and rounded once"""
    x = np.asarray(x)
    if x.ndim == 2:
        x = x[:, :, None]
    T, C, Q = x.shape
    out = {k: np.zeros((C, Q)) for k in ("x0", "s1", "s1a", "s1b", "m2a", "m2b")}
    out["p"] = np.zeros((C, Q, L + 1))
    for c in range(C):
        for q in range(Q):
            r1 = pass1(x[:, c, q])
            s1, s1a, s1b = r1["s1"][0], r1["s1a"][0], r1["s1b"][0]
            r2 = pass2(r1["d"], *means(T, s1, s1a, s1b), L=L)
            out["x0"][c, q], out["s1"][c, q], out["s1a"][c, q], out["s1b"][c, q] = r1["x0"], s1, s1a, s1b
            out["m2a"][c, q], out["m2b"][c, q] = r2["m2a"][0], r2["m2b"][0]
            out["p"][c, q] = [v for v, _ in r2["p"]]
    out["T"], out["maxlag"] = T, L
    return out


def variance(v):
    """ddof 1"""
    mu = math.fsum(v) / len(v)
    return math.fsum((t - mu) ** 2 for t in v) / (len(v) - 1)


def geyer(rho):
    """(tau, cut, truncated) of rho[0..L]: pairs G_j = rho_2j + rho_2j+1, cut at the first non-positive one, made monotone"""
    npairs = len(rho) // 2
    if npairs < 1:
        return float("nan"), 0, True
    G = []
    for j in range(npairs):
        g = rho[2 * j] + rho[2 * j + 1]
        if not g > 0:
            break
        G.append(g)
    cut = len(G)
    for j in range(1, cut):
        G[j] = min(G[j], G[j - 1])
    return -1.0 + 2.0 * math.fsum(G), cut, cut == npairs


def rho_table(p, mean, n):
    """rho_k, k = 0..L of the chains with lag sums p[m][L+1] and the means mean[m]"""
    m = len(p)
    Wn = math.fsum(float(pc[0]) for pc in p) / m / (n - 1)
    Bn = variance([float(v) for v in mean]) if m > 1 else 0.0
    varp = (n - 1) / n * Wn + Bn
    return [1.0 - (Wn - math.fsum(float(pc[k]) for pc in p) / m / n) / varp for k in range(len(p[0]))]


def convergence(tab, chains, q):
    """dict of rhat, ess, tau, cut, truncated, constant, and per chain mean, std, chain_tau for column q over `chains` (positions)"""
    n, L = tab["T"], tab["maxlag"]
    h = n // 2
    m = len(chains)
    nan = float("nan")
    out = dict(rhat=nan, ess=nan, tau=nan, cut=0, truncated=False, constant=False, mean=[nan] * m, std=[nan] * m, chain_tau=[nan] * m)
    if not m:
        return out
    out["mean"] = [float(tab["x0"][c, q]) + float(tab["s1"][c, q]) / n for c in chains]
    if n > 1:
        out["std"] = [math.sqrt(float(tab["p"][c, q, 0]) / (n - 1)) for c in chains]
    out["constant"] = all(float(tab["p"][c, q, 0]) == 0.0 for c in chains)
    if n < 4 or out["constant"]:
        return out
    m2 = [float(tab["m2a"][c, q]) for c in chains] + [float(tab["m2b"][c, q]) for c in chains]
    W = math.fsum(v / (h - 1) for v in m2) / (2 * m)
    hm = [float(tab["x0"][c, q]) + float(tab["s1a"][c, q]) / h for c in chains] + \
         [float(tab["x0"][c, q]) + float(tab["s1b"][c, q]) / h for c in chains]
    out["rhat"] = math.sqrt(((h - 1) / h * W + variance(hm)) / W)
    p = [tab["p"][c, q] for c in chains]
    tau, cut, trunc = geyer(rho_table(p, out["mean"], n))
    out["tau"], out["cut"], out["truncated"] = tau, cut, trunc
    out["ess"] = m * n / max(tau, 1.0 / math.log10(m * n))
    for j, c in enumerate(chains):
        if float(tab["p"][c, q, 0]) > 0:
            out["chain_tau"][j] = geyer(rho_table([tab["p"][c, q]], [out["mean"][j]], n))[0]
    return out


def pair_sums(tab, chains, q):
    """Geyer's pair sums G_j of column q (before the cut): the GPU test picks inputs whose G stay clear of zero at the cut"""
    rho = rho_table([tab["p"][c, q] for c in chains], [float(tab["x0"][c, q]) + float(tab["s1"][c, q]) / tab["T"] for c in chains], tab["T"])
    return [rho[2 * j] + rho[2 * j + 1] for j in range(len(rho) // 2)]


def ar1(rs, T, C, phi, Q=None):
    """stationary AR(1) series of unit innovation variance: [T][C] or [T][C][Q]"""
    shape = (T, C) if Q is None else (T, C, Q)
    z = rs.standard_normal(shape)
    x = np.empty(shape)
    x[0] = z[0] / math.sqrt(1.0 - phi * phi)
    for t in range(1, T):
        x[t] = phi * x[t - 1] + z[t]
    return x
