"""A plain restatement of the evidence estimates of tempered runs (include/bh_engine_chain_ladder_evidence.h,
bayhunter_amd.diagnostics.ladder_holders / ladder_evidence) that imports nothing of the package: loops over Python floats.

beta[t][c]: the recorded betas; likes[t][c]: the recorded log-likelihoods; ladder[c]: any integer ids.  Series j = start[k] + r is
rung r of ladder k (rung 0 cold), start the prefix sum of the ladder sizes in ascending id, chains ascending within a ladder.
    hold[t][j]  = the chain of ladder k with #{larger betas among the ladder's chains at row t} == r
    b_j         = the beta at series j, the same bits at every row
    l_j[t]      = float(likes[t][hold[t][j]]);  mx_j, mn_j = its largest and smallest value
    Df_j        = b_{j-1} - b_j (0 at rung 0);  Dr_j = b_j - b_{j+1} (0 at the hottest rung)
    wf          = exp(Df_j * (l - mx_j)),  wr = exp(-Dr_j * (l - mn_j)),  a term whose argument is <= -512 exactly 0
    Sf, Sf2, Sr, Sr2 = the sums of wf, wf * wf, wr, wr * wr in 16 strands (strand s: the rows t = s mod 16, ascending, from 0),
                  combined (((s0+s1)+(s2+s3))+((s4+s5)+(s6+s7)))+(((s8+s9)+(s10+s11))+((s12+s13)+(s14+s15)))
exp is math.exp: the host libm's, one call per term (numpy's vectorised exp is another routine with other bits).

The estimates of a ladder with betas b_0 > ... > b_{R-1}, T rows, D_r = b_{r-1} - b_r, and U_r, V_r, N_r the mean, the variance
P_0 / T and the effective sample size of rung r's series:
    log_ratio[r-1]     = log(Sf_r / T) + D_r * mx_r                    r = 1..R-1
    log_ratio_rev[r-1] = -(log(Sr_{r-1} / T) - D_r * mn_{r-1})
    ss, ss_rev         = their sums, added in ascending r from 0.0
    ss_err             = sqrt(sum_r (T * Sf2_r / (Sf_r * Sf_r) - 1) / N_r),  ss_rev_err with Sr, Sr2 and N of rung r-1
    ti                 = sum_r D_r * (U_{r-1} + U_r) / 2
    ti2                = ti - sum_r D_r * D_r / 12 * (V_{r-1} - V_r)
    ti_err             = sqrt(sum_r w_r * w_r * V_r / N_r),  w the trapezoid weights (D_r / 2 to either end of every step)
    beta_min = b_{R-1},  complete = (beta_min == 0.0)
"""
import math

import numpy as np

import diag_ref

STRANDS = 16
DROP = -512.0
SUMS = ("mx", "mn", "sf", "sf2", "sr", "sr2")


def ladders(ladder):
    ladder = [int(v) for v in np.asarray(ladder).reshape(-1)]
    ids = sorted(set(ladder))
    return ids, [[c for c in range(len(ladder)) if ladder[c] == lid] for lid in ids]


def holders(beta, ladder):
    """ids, members, hold int32 [T][C], rung_beta [C]; ValueError with the engine's words for data it refuses"""
    beta = np.asarray(beta, dtype=np.float64)
    T, C = beta.shape
    ids, members = ladders(ladder)
    assert sum(len(m) for m in members) == C
    if not np.all(np.isfinite(beta)):
        raise ValueError("a beta is not finite")
    hold = np.full((T, C), -1, np.int32)
    start = 0
    for m in members:
        b = beta[:, m]                                                  # [T][R]
        rung = (b[:, None, :] > b[:, :, None]).sum(axis=2)             # rung[t][i] = #{i' : b[t][i'] > b[t][i]}
        if np.any((b[:, None, :] == b[:, :, None]).sum(axis=2) > 1):
            raise ValueError("tied betas")
        for i, c in enumerate(m):
            hold[np.arange(T), start + rung[:, i]] = c
        start += len(m)
    assert hold.min() >= 0
    held = np.take_along_axis(beta, hold.astype(np.int64), 1)
    if np.any(held.view(np.uint64) != held[:1].view(np.uint64)):
        raise ValueError("the betas of a ladder change within the rows")
    return np.array(ids, dtype=np.int64), [np.array(m, dtype=np.int64) for m in members], hold, held[0].copy()


def strand_sum(terms):
    """the sum of the terms (one per row, in row order) in the 16 strands and their tree"""
    s = [0.0] * STRANDS
    for t, v in enumerate(terms):
        s[t % STRANDS] += v
    return (((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]))) + \
           (((s[8] + s[9]) + (s[10] + s[11])) + ((s[12] + s[13]) + (s[14] + s[15])))


def term(a):
    return 0.0 if a <= DROP else math.exp(a)


def series_terms(l, mx, mn, df, dr):
    """(wf, wr) per row of one series: l the likes as Python floats"""
    return [term(df * (v - mx)) for v in l], [term(-dr * (v - mn)) for v in l]


def sums(beta, likes, ladder):
    """dict of ids, members, hold, rung_beta, T and mx, mn, sf, sf2, sr, sr2 [C]"""
    likes = np.asarray(likes)
    if not np.all(np.isfinite(likes)):
        raise ValueError("a like is not finite")
    ids, members, hold, rb = holders(beta, ladder)
    T, C = hold.shape
    out = {k: np.zeros(C) for k in SUMS}
    start = 0
    for m in members:
        R = len(m)
        for r in range(R):
            j = start + r
            l = [float(likes[t, hold[t, j]]) for t in range(T)]
            mx, mn = max(l), min(l)
            df = float(rb[j - 1]) - float(rb[j]) if r >= 1 else 0.0
            dr = float(rb[j]) - float(rb[j + 1]) if r <= R - 2 else 0.0
            wf, wr = series_terms(l, mx, mn, df, dr)
            out["mx"][j], out["mn"][j] = mx, mn
            out["sf"][j], out["sf2"][j] = strand_sum(wf), strand_sum([v * v for v in wf])
            out["sr"][j], out["sr2"][j] = strand_sum(wr), strand_sum([v * v for v in wr])
        start += R
    out.update(ids=ids, members=members, hold=hold, rung_beta=rb, T=T)
    return out


def estimates(T, b, s, U, V, N):
    """the estimates of one ladder (module docstring): b [R], s = dict of the six sums [R], U, V, N [R]; Python floats throughout"""
    R = len(b)
    b = [float(v) for v in b]
    s = {k: [float(v) for v in s[k]] for k in SUMS}
    U, V, N = [float(v) for v in U], [float(v) for v in V], [float(v) for v in N]
    n = float(T)
    nan = float("nan")
    fwd, rev = [], []
    vf = vr = ti = corr = 0.0
    w = [0.0] * R
    for r in range(1, R):
        d = b[r - 1] - b[r]
        fwd.append(math.log(s["sf"][r] / n) + d * s["mx"][r])
        rev.append(-(math.log(s["sr"][r - 1] / n) - d * s["mn"][r - 1]))
        vf += (n * s["sf2"][r] / (s["sf"][r] * s["sf"][r]) - 1.0) / N[r]
        vr += (n * s["sr2"][r - 1] / (s["sr"][r - 1] * s["sr"][r - 1]) - 1.0) / N[r - 1]
        ti += d * (U[r - 1] + U[r]) / 2.0
        corr += d * d / 12.0 * (V[r - 1] - V[r])
        w[r - 1] += d / 2.0
        w[r] += d / 2.0
    te = 0.0
    for r in range(R):
        if w[r] != 0.0:
            te += w[r] * w[r] * V[r] / N[r]
    ss = ss_rev = 0.0
    for v in fwd:
        ss += v
    for v in rev:
        ss_rev += v
    root = lambda v: math.sqrt(v) if v >= 0.0 else nan      # (a NaN ESS -- a constant series, T < 4 -- gives a NaN error)
    return dict(log_ratio=np.array(fwd, dtype=np.float64), log_ratio_rev=np.array(rev, dtype=np.float64), ss=ss, ss_err=root(vf),
                ss_rev=ss_rev, ss_rev_err=root(vr), ti=ti, ti2=ti - corr, ti_err=root(te), beta_min=b[R - 1], complete=b[R - 1] == 0.0)


def series_stats(gathered, L):
    """mean, var, tau, ess, rhat, ess_truncated [C] of the series gathered[t][j] by the restatement tests/diag_ref.py (every sum exact
    and rounded once: the numbers of the package within the bounds stated there, not its bits)"""
    tab = diag_ref.tables(np.asarray(gathered), L)
    T, C = gathered.shape
    out = {k: [] for k in ("mean", "var", "tau", "ess", "rhat", "ess_truncated")}
    for j in range(C):
        c = diag_ref.convergence(tab, [j], 0)
        out["mean"].append(c["mean"][0])
        out["var"].append(float(tab["p"][j, 0, 0]) / T)
        for k in ("tau", "ess", "rhat"):
            out[k].append(c[k])
        out["ess_truncated"].append(c["truncated"])
    return out


def evidence(beta, likes, ladder, maxlag=None, stats=series_stats):
    """the dict of bayhunter_amd.diagnostics.ladder_evidence; stats(gathered [T][C], L): the numbers of the rung series"""
    out = sums(beta, likes, ladder)
    T = out["T"]
    L = min(T // 2, 1000) if maxlag is None else int(maxlag)
    st = stats(np.take_along_axis(np.asarray(likes), out["hold"].astype(np.int64), 1), L)
    out["maxlag"], out["ladders"] = L, []
    start = 0
    for m in out["members"]:
        sl = slice(start, start + len(m))
        start += len(m)
        d = estimates(T, out["rung_beta"][sl], {k: out[k][sl] for k in SUMS}, st["mean"][sl], st["var"][sl], st["ess"][sl])
        d["betas"] = out["rung_beta"][sl].copy()
        for k in ("mean", "var", "tau", "ess", "rhat"):
            d[k] = np.array(st[k][sl], dtype=np.float64)
        d["ess_truncated"] = np.array(st["ess_truncated"][sl], dtype=bool)
        out["ladders"].append(d)
    return out


# ---- the analytic ladder ----------------------------------------------------------------------------------------------------------
ANALYTIC_BETAS = (1.0, 0.6, 0.35, 0.2, 0.12, 0.07, 0.04, 0.02, 0.01, 0.005, 0.002, 0.0)
ANALYTIC_LOGZ = -2.0 * math.log(101.0)


def analytic_ladder(seed, T=2048):
    """theta in R^4, prior N(0, I), log L = -|theta|^2 / (2 * 0.01): at beta the posterior is N(0, I / (1 + 100 beta)) and
    log Z(beta) = -2 log(1 + 100 beta).  T independent draws per rung of ANALYTIC_BETAS, the likes stored as float32, every row's
    betas (and likes with them) permuted over the 12 chains.  Returns beta [T][12] float64, likes [T][12] float32, ladder [12]."""
    rs = np.random.RandomState(seed)
    R = len(ANALYTIC_BETAS)
    beta, likes = np.zeros((T, R)), np.zeros((T, R), np.float32)
    ll = np.zeros((T, R))
    for r, b in enumerate(ANALYTIC_BETAS):
        theta = rs.standard_normal((T, 4)) / math.sqrt(1.0 + 100.0 * b)
        ll[:, r] = -np.sum(theta * theta, axis=1) / (2.0 * 0.01)
    for t in range(T):
        perm = rs.permutation(R)            # chain perm[r] holds rung r
        beta[t, perm] = ANALYTIC_BETAS
        likes[t, perm] = ll[t]
    return beta, likes, np.zeros(R, np.int64)


def within_errors(d, nerr=4.0):
    """the three conditions of the analytic ladder on one ladder's dict: (name, value, error, distance in errors) per estimate"""
    rows = [("ss", d["ss"], d["ss_err"]), ("ss_rev", d["ss_rev"], d["ss_rev_err"]), ("ti2", d["ti2"], d["ti_err"])]
    return [(k, v, e, abs(v - ANALYTIC_LOGZ) / e) for k, v, e in rows]
