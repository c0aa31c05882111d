"""A plain numpy restatement of the rank transform (include/bh_engine_chain_rank.h, bayhunter_amd/diagnostics.py): the counts with
numpy.unique, the fold about numpy.median, the tail indicators from the integer rule.  Only the table of normal scores comes from
the package (diagnostics.rank_table: it is the definition of the scores, tested against the standard library on its own)."""
import numpy as np

from bayhunter_amd.diagnostics import rank_table


def counts(pool):
    """(lt, eq) of every element of a 1-D pool: the elements below it and equal to it (itself included)"""
    _, inv, cnt = np.unique(pool, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    return (np.cumsum(cnt) - cnt)[inv], cnt[inv]


def r2(pool):
    """twice the average rank"""
    lt, eq = counts(pool)
    return 2 * lt + eq + 1


def rank_pool(pool, zt=None):
    """(z, zf, lo, hi) of a 1-D pool (any float dtype)"""
    v = np.asarray(pool).astype(np.float64) + 0.0          # -0.0 + 0.0 is +0.0
    N = v.size
    zt = rank_table(N) if zt is None else zt
    lt, eq = counts(v)
    z = zt[2 * lt + eq + 1]
    lo = (lt <= (N - 1) // 20).astype(np.float32)
    hi = (lt <= (19 * (N - 1)) // 20).astype(np.float32)
    f = np.abs(v - np.median(v))
    ltf, eqf = counts(f)
    return z, zt[2 * ltf + eqf + 1], lo, hi


def rank_tables(x, group):
    """(z, zf float64 [T][C][Q], tail float32 [T][C][2Q]) of a table x [T][C][Q] with the pools group[c] (-1: left out, zeros)"""
    x = np.asarray(x)
    if x.ndim == 2:
        x = x[:, :, None]
    T, C, Q = x.shape
    group = np.asarray(group)
    z, zf, tail = np.zeros((T, C, Q)), np.zeros((T, C, Q)), np.zeros((T, C, 2 * Q), np.float32)
    for g in range(int(group.max()) + 1):
        cs = np.flatnonzero(group == g)
        zt = rank_table(T * cs.size)
        for q in range(Q):
            a, b, lo, hi = rank_pool(x[:, cs, q].reshape(-1), zt)
            z[:, cs, q], zf[:, cs, q] = a.reshape(T, cs.size), b.reshape(T, cs.size)
            tail[:, cs, 2 * q], tail[:, cs, 2 * q + 1] = lo.reshape(T, cs.size), hi.reshape(T, cs.size)
    return z, zf, tail
