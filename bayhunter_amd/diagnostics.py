"""Convergence of every site's chains: outlier chains, split R-hat and effective sample size.

The reference answers "which chains may be summarised, and have they converged?" with PlotFromStorage.get_outliers and the
plot_iiter* trace plots a person reads for one station.  Here the numbers come per station and per parameter, from the
time-ordered tables of the chains' thinned samples -- [rows][C][..], one column per chain, which is what record="device" writes
(DeviceChains.samples_dev) and what the saved c???_p2*.npy files stack to.

Three layers:

chain_series_stats / chain_model_stats -- the GPU part (include/bh_engine_chain_diag.h).  Per series (chain c, column q) of T
    samples x_i, in float64:  x0 = x_0,  d_i = x_i - x0,  h = T // 2,  the halves i < h and i >= T - h,
        S1 = sum d_i,  S1a, S1b = the halves' sums,
        m = S1 / T,  ma = S1a / h,  mb = S1b / h,
        M2a = sum_{first half} (d_i - ma)^2,  M2b likewise,
        P_k = sum_{i < T-k} e_i e_{i+k},  e_i = d_i - m,  k = 0..maxlag  (0 for k >= T),
    every sum in an order that depends on (T, maxlag) only, so a series has the same bits wherever it stands.

convergence -- pure numpy on those tables.  For a site with the kept chains c = 1..m, n = T, per column:
    per chain   mean_c = x0 + S1 / n,   std_c = sqrt(P_0 / (n - 1)),
                tau_c  = the estimator below with this chain alone (m = 1).
    split R-hat over the 2m half chains:
                W    = mean over the halves of M2 / (h - 1)
                B/h  = the variance (ddof 1) of the 2m half means  x0 + S1a / h,  x0 + S1b / h
                rhat = sqrt(((h - 1) / h * W + B/h) / W)
    ESS (Stan's multi-chain estimator, on the unsplit chains):
                W_n   = mean_c P_{c,0} / (n - 1)
                B/n   = the variance (ddof 1) of the m chain means (0 for m = 1)
                var+  = (n - 1) / n * W_n + B/n
                rho_k = 1 - (W_n - mean_c P_{c,k} / n) / var+,      k = 0..maxlag
                G_j   = rho_{2j} + rho_{2j+1},                       j = 0..(maxlag + 1) // 2 - 1   (Geyer's pairs)
                cut   = the first j with G_j <= 0 (the number of pairs if there is none: then ess_truncated)
                G_j   = min(G_j, G_{j-1}) for 0 < j < cut           (monotone)
                tau   = -1 + 2 * sum_{j < cut} G_j
                ess   = m n / max(tau, 1 / log10(m n))               (the cap at m n log10(m n))
    constant: every kept chain has P_0 == 0 -- rhat, ess and tau are NaN (a fixed vpvs, a fixed correlation, an absent slot).
    T < 4, no kept chain, or no pair (maxlag < 1, for ess and tau): NaN, not an error.

outlier_chains -- the reference's rule (Plotting.get_outliers, results.get_outliers) per site: the chains whose median likelihood
    deviates from the site's best chain's by more than `dev`.

Tempered runs (include/bh_engine_chain_diag_ladders.h): no chain's recorded series is a posterior series -- a ladder's cold state moves
between its chains.  The posterior series of ladder k is its cold series: at row t the state of chain sel[t][k], the first chain of
the ladder that holds its largest beta (parallel.cold_samples' pick).  ladder_index forms sel on the GPU from the recorded betas,
with the numbers that say whether the ladder mixes; chain_series_stats, chain_model_stats, chain_medians and diagnose take sel= and
then describe K series, one per ladder, that read chain sel[t][k] at row t from the tables where they lie.  Every output has the bits
of the same call on the table gathered on the host, np.take_along_axis(x, sel, 1).  ladder_index, all in integers, with M(c) the
chains of c's ladder:
    rung[t][c]      = #{c' in M(c) : beta[t][c'] > beta[t][c]}       (0 is cold; ties share a rung)
    sel[t][k]       = min{c in ladder k : rung[t][c] == 0}
    hot             : no chain of M(c) has a smaller beta and rung[t][c] > 0
    occupancy[c][r] = #{t : rung[t][c] == r}
    round_trips[c]  = the cold -> hot -> cold excursions seen at the recorded rows
    moves[k]        = #{t >= 1 : sel[t][k] != sel[t-1][k]}

Rank-normalised numbers (Vehtari et al. 2021; include/bh_engine_chain_rank.h): rank_series / rank_models turn every column of a
table into three tables on the GPU, with the samples of a site's kept chains pooled per column (N = m T values, -0.0 as +0.0):
    lt = #{w in pool : w < v},  eq = #{w in pool : w == v},  R2 = 2 lt + eq + 1   (twice the average rank; integers throughout)
    z    = rank_table(N)[R2]  = normal_quantile((R2/2 - 3/8) / (N + 1/4))         (bulk)
    zf   = the same of f = |v - numpy.median(pool)|                              (folded: spread instead of location)
    tail = lt <= (N - 1) // 20,  lt <= 19 (N - 1) // 20                          (x <= q_0.05, x <= q_0.95 of numpy.quantile)
rank_convergence feeds those tables to chain_series_stats and convergence, unchanged: rhat_bulk = the split R-hat of z, rhat_fold
of zf, rhat the larger; ess_bulk the ESS of z, ess_tail the smaller of the ESS of the two indicators.  The ESS stays the package's:
Stan's estimator on the UNSPLIT chains (`posterior` and ArviZ split every chain in two for the ESS as well; here only R-hat does).
The normal scores are a host table (AS241), looked up on the device: the tables have the host's bits.

The evidence of tempered runs (include/bh_engine_chain_ladder_evidence.h): ladder_holders finds, on the GPU, the chain that holds every
rung of every ladder at every row -- hold[t][j], a sel= with one series per temperature --, and ladder_evidence forms from the
recorded likes of the rung series the log ratios Z(b_{r-1}) / Z(b_r) of neighbouring rungs (stepping stones in both directions) and the
thermodynamic integral, with errors from the rung series' ESS; formulas and caveats in its docstring.

Structural features (include/bh_engine_chain_diag_features.h): the numbers an array study publishes -- a Moho depth, a sediment
thickness, the probability of a low-velocity zone -- are functionals of the model rows that posterior_features forms on rows which
have lost their time order.  chain_feature_series forms the same columns, bit for bit, as series of every chain from the store where
it lies: value (0 where a row lacks the feature), present (the indicator) and missing (the counts); feature_convergence gives every
column R-hat, ESS and a Monte-Carlo standard error, with a stated rule for the rows that lack it (its docstring); diagnose takes
features= / moho=.

Not here: ranks of the cold series of tempered runs (sel=), ladders spread over ranks, chains spread over ranks.
"""
import ctypes as C
import math

import numpy as np

from . import engine as E
from .posterior import median_of_middles

FIELDS = ("x0", "s1", "s1a", "s1b", "m2a", "m2b")


def _is_tensor(a):
    try:
        import torch
    except ImportError:
        return False
    return isinstance(a, torch.Tensor)


def _table(values):
    """(pointer, memspace, stream, elem_bytes, shape, strides in elements, keep-alive) of a [T][C] or [T][C][Q] table: a numpy
    array or a device torch tensor, read where it lies when its last axis is contiguous (else copied once)"""
    if _is_tensor(values):
        import torch
        if not values.is_cuda or values.dtype not in (torch.float32, torch.float64) or values.dim() not in (2, 3):
            raise ValueError("a table is a [T][C] or [T][C][Q] float32/float64 array or device tensor")
        if values.dim() == 3 and values.shape[2] > 1 and values.stride(2) != 1:
            values = values.contiguous()
        if min(values.stride()[:2]) < 1 and values.shape[0] > 1 and values.shape[1] > 1:
            values = values.contiguous()
        stream = C.c_void_p(torch.cuda.current_stream(values.device).cuda_stream)
        return C.c_void_p(values.data_ptr()), E.DEVICE, stream, values.element_size(), tuple(values.shape), tuple(values.stride()), values
    a = np.asarray(values)
    if a.dtype not in (np.float32, np.float64) or a.ndim not in (2, 3):
        raise ValueError("a table is a [T][C] or [T][C][Q] float32/float64 array or device tensor")
    st = a.strides
    ok = all(s % a.itemsize == 0 and s > 0 for s in st[:2]) and (a.ndim == 2 or a.shape[2] == 1 or st[2] == a.itemsize)
    if not ok:
        a = np.ascontiguousarray(a)
    strides = tuple(s // a.itemsize for s in a.strides)
    return C.c_void_p(a.ctypes.data), E.HOST, None, a.itemsize, a.shape, strides, a


def _engine(engine):
    return engine if engine is not None else E.default_engine(0)


def _outputs(Cn, Q, L):
    out = {k: np.zeros((Cn, Q)) for k in FIELDS}
    out["p"] = np.zeros((Cn, Q, L + 1))
    return out


def _lds(shape, strides, width):
    """ld_t, ld_c of a table; an axis of length 1 has no stride of its own"""
    T, Cn = shape[:2]
    ld_c = strides[1] if Cn > 1 else width
    ld_t = strides[0] if T > 1 else max(1, ld_c * Cn)
    return int(ld_t), int(ld_c)


def _sel_table(sel, T, Cn, mem):
    """(pointer, K, ld_sel, keep-alive) of a selection sel[t][k]: int32, numpy for a numpy table and a device tensor for a device one,
    read where it lies when its rows are contiguous"""
    if mem == E.DEVICE:
        import torch
        if not _is_tensor(sel) or not sel.is_cuda:
            raise ValueError("sel of a device table is a device tensor")
        if sel.dim() != 2 or sel.shape[0] != T or sel.shape[1] < 1:
            raise ValueError("sel: [T][K], K >= 1")
        if sel.dtype != torch.int32:
            sel = sel.to(torch.int32)
        if (sel.shape[1] > 1 and sel.stride(1) != 1) or (T > 1 and sel.stride(0) < sel.shape[1]):
            sel = sel.contiguous()
        K = int(sel.shape[1])
        return C.c_void_p(sel.data_ptr()), K, (int(sel.stride(0)) if T > 1 else K), sel
    if _is_tensor(sel):
        raise ValueError("sel of a numpy table is a numpy array")
    a = np.asarray(sel)
    if a.ndim != 2 or a.shape[0] != T or a.shape[1] < 1 or a.dtype.kind not in "iu":
        raise ValueError("sel: [T][K] integers, K >= 1")
    if a.dtype != np.int32:
        if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise ValueError("sel: an index beyond int32")
        a = a.astype(np.int32)
    K = int(a.shape[1])
    if (K > 1 and a.strides[1] != 4) or (T > 1 and (a.strides[0] % 4 or a.strides[0] < 4 * K)):
        a = np.ascontiguousarray(a)
    return C.c_void_p(a.ctypes.data), K, (a.strides[0] // 4 if T > 1 else K), a


def _ladders(ladder):
    """ids [K], the chains' positions among them [C] (int32), members per ladder, R of any integer ladder ids"""
    ladder = np.asarray(ladder).reshape(-1)
    ids, inv = np.unique(ladder, return_inverse=True)
    inv = np.ascontiguousarray(inv.reshape(-1), dtype=np.int32)
    K = int(ids.size)
    counts = np.bincount(inv, minlength=K)
    members = np.split(np.argsort(inv, kind="stable"), np.cumsum(counts)[:-1]) if K else []      # ascending chains per ladder
    return ids, inv, members, (int(counts.max()) if K else 0)


def _beta_table(beta, Cn):
    """(pointer, memspace, stream, T, ld_t, keep-alive) of the recorded betas [T][C]: float64, a numpy array or a device tensor, read
    where it lies when its rows are contiguous (else copied once)"""
    if _is_tensor(beta):
        import torch
        if not beta.is_cuda or beta.dtype != torch.float64 or beta.dim() != 2:
            raise ValueError("beta: a [T][C] float64 array or device tensor")
        T = int(beta.shape[0])
        if (beta.shape[1] > 1 and beta.stride(1) != 1) or (T > 1 and beta.stride(0) < beta.shape[1]):
            beta = beta.contiguous()
        ptr, mem, ld_t = C.c_void_p(beta.data_ptr()), E.DEVICE, (int(beta.stride(0)) if T > 1 else max(1, int(beta.shape[1])))
        stream = C.c_void_p(torch.cuda.current_stream(beta.device).cuda_stream)
        shape = tuple(beta.shape)
    else:
        beta = np.asarray(beta)
        if beta.dtype != np.float64 or beta.ndim != 2:
            raise ValueError("beta: a [T][C] float64 array or device tensor")
        T = int(beta.shape[0])
        if (beta.shape[1] > 1 and beta.strides[1] != 8) or (T > 1 and (beta.strides[0] % 8 or beta.strides[0] < 8 * beta.shape[1])):
            beta = np.ascontiguousarray(beta)
        ptr, mem, stream, ld_t = C.c_void_p(beta.ctypes.data), E.HOST, None, (beta.strides[0] // 8 if T > 1 else max(1, beta.shape[1]))
        shape = beta.shape
    if T < 1 or Cn < 1 or shape[1] != Cn:
        raise ValueError("beta [T][C] and ladder [C]: T >= 1, one ladder id per chain")
    return ptr, mem, stream, T, int(ld_t), beta


def ladder_index(beta, ladder, engine=None):
    """The cold chain of every ladder at every recorded row, and how the ladders mix (module docstring; bh_chain_ladder_index).
    beta[t][c]: the recorded betas, float64, a numpy array or a device tensor (a strided view of the store is read where it lies);
    ladder[c]: any integer ladder ids.  Dict of ids [K] (the sorted ladder ids, the order of sel's columns), members (per ladder
    the positions of its chains), sel int32 [T][K] and rung int32 [T][C] (device tensors for a device beta, numpy otherwise),
    occupancy int64 [C][R] (R = the largest ladder's size), round_trips int64 [C], moves int64 [K].  EngineError: a ladder of more
    than 64 chains, a beta that is not finite."""
    eng = _engine(engine)
    ids, inv, members, R = _ladders(ladder)
    Cn, K = int(inv.size), int(ids.size)
    ptr, mem, stream, T, ld_t, beta = _beta_table(beta, Cn)
    if mem == E.DEVICE:
        import torch
        sel = torch.full((T, K), -1, dtype=torch.int32, device=beta.device)
        rung = torch.full((T, Cn), -1, dtype=torch.int32, device=beta.device)
        psel, prung = C.c_void_p(sel.data_ptr()), C.c_void_p(rung.data_ptr())
    else:
        sel, rung = np.full((T, K), -1, np.int32), np.full((T, Cn), -1, np.int32)
        psel, prung = E._ptr(sel), E._ptr(rung)
    occ, trips, moves = np.zeros((Cn, max(R, 1)), np.int64), np.zeros(Cn, np.int64), np.zeros(K, np.int64)
    eng._check(eng._L.bh_chain_ladder_index(eng._h, mem, stream, T, Cn, ld_t, ptr, E._ptr(inv), K, R, psel, K, prung, Cn,
                                            E._ptr(occ), E._ptr(trips), E._ptr(moves)))
    del beta
    return dict(ids=ids, members=members, sel=sel, rung=rung, occupancy=occ, round_trips=trips, moves=moves)


def _hold_table(beta, mem, T, Cn):
    """hold int32 [T][C] beside the betas: a device tensor for a device beta, numpy otherwise"""
    if mem == E.DEVICE:
        import torch
        hold = torch.full((T, Cn), -1, dtype=torch.int32, device=beta.device)
        return hold, C.c_void_p(hold.data_ptr())
    hold = np.full((T, Cn), -1, np.int32)
    return hold, E._ptr(hold)


def ladder_holders(beta, ladder, engine=None):
    """The chain that holds every rung of every ladder at every recorded row (include/bh_engine_chain_ladder_evidence.h;
    bh_chain_ladder_holders).  beta, ladder: as in ladder_index.  Returns ids [K], members (per ladder the positions of its chains),
    hold int32 [T][C] (a device tensor for a device beta, numpy otherwise) and rung_beta [C]: series j = start[k] + r is rung r of
    ladder k -- the concatenated members number the series --, hold[t][j] the chain at that rung at row t, rung_beta[j] the beta
    it holds, descending within a ladder.  hold is a sel= of chain_series_stats, chain_model_stats and chain_medians: the series
    of every temperature, the cold ones (r = 0) among them.  EngineError: a ladder of more than 64 chains, a beta that is not
    finite, tied betas in a ladder, betas that change within the rows."""
    eng = _engine(engine)
    ids, inv, members, R = _ladders(ladder)
    Cn, K = int(inv.size), int(ids.size)
    ptr, mem, stream, T, ld_t, beta = _beta_table(beta, Cn)
    hold, phold = _hold_table(beta, mem, T, Cn)
    rung_beta = np.zeros(Cn)
    eng._check(eng._L.bh_chain_ladder_holders(eng._h, mem, stream, T, Cn, ld_t, ptr, E._ptr(inv), K, R, phold, Cn, E._ptr(rung_beta)))
    del beta
    return ids, members, hold, rung_beta


EVIDENCE_SUMS = ("mx", "mn", "sf", "sf2", "sr", "sr2")


def ladder_evidence_sums(beta, likes, ladder, engine=None):
    """The engine call behind ladder_evidence (bh_chain_ladder_evidence): dict of ids, members, hold, rung_beta as ladder_holders
    returns them, T, and per series j (float64 [C]) mx, mn -- the largest and smallest like of the rung's series --, sf, sf2, sr,
    sr2 -- the sums of exp(Df (l - mx)), of its square, of exp(-Dr (l - mn)) and of its square over the series, Df / Dr the step of
    beta to the colder / the hotter rung (0 at a ladder's ends), in the 16 strands of chain_series_stats."""
    eng = _engine(engine)
    ids, inv, members, R = _ladders(ladder)
    Cn, K = int(inv.size), int(ids.size)
    ptr, mem, stream, T, ld_t, beta = _beta_table(beta, Cn)
    xptr, xmem, _, elem, shape, strides, keep = _table(likes)
    if len(shape) != 2 or tuple(shape) != (T, Cn):
        raise ValueError("likes: [T][C], the shape of beta")
    if xmem != mem:
        raise ValueError("beta and likes: both numpy arrays or both device tensors")
    if mem == E.DEVICE and keep.device != beta.device:
        raise ValueError("beta and likes lie on different devices")
    ldx_t, ldx_c = _lds(shape, strides, 1)
    hold, phold = _hold_table(beta, mem, T, Cn)
    out = {k: np.zeros(Cn) for k in ("rung_beta",) + EVIDENCE_SUMS}
    eng._check(eng._L.bh_chain_ladder_evidence(eng._h, mem, stream, T, Cn, ld_t, ptr, elem, ldx_t, ldx_c, xptr, E._ptr(inv), K, R,
                                               phold, Cn, *[E._ptr(out[k]) for k in ("rung_beta",) + EVIDENCE_SUMS]))
    del beta, keep
    out.update(ids=ids, members=members, hold=hold, T=T)
    return out


def evidence_estimates(T, betas, sums, mean, var, ess):
    """The estimates of one ladder of R rungs from its series' numbers, all Python floats (math.log, math.sqrt): betas [R] descending,
    sums = dict of mx, mn, sf, sf2, sr, sr2 [R], mean, var, ess [R] of the rung series.  Formulas: ladder_evidence."""
    R = len(betas)
    b = [float(v) for v in betas]
    s = {k: [float(v) for v in sums[k]] for k in EVIDENCE_SUMS}
    U, V, N = [float(v) for v in mean], [float(v) for v in var], [float(v) for v in ess]
    nan = float("nan")
    n = float(T)

    def log_or_nan(v):
        return math.log(v) if v > 0.0 else nan

    def root_or_nan(v):
        return math.sqrt(v) if v >= 0.0 else nan

    fwd, rev, vf, vr = [], [], 0.0, 0.0
    for r in range(1, R):          # the pair (r - 1, r): forward from the hotter rung r, reverse from the colder rung r - 1
        d = b[r - 1] - b[r]
        fwd.append(log_or_nan(s["sf"][r] / n) + d * s["mx"][r])
        rev.append(-(log_or_nan(s["sr"][r - 1] / n) - d * s["mn"][r - 1]))
        vf += (n * s["sf2"][r] / (s["sf"][r] * s["sf"][r]) - 1.0) / N[r]
        vr += (n * s["sr2"][r - 1] / (s["sr"][r - 1] * s["sr"][r - 1]) - 1.0) / N[r - 1]
    ti = ti2 = 0.0
    w = [0.0] * R
    for r in range(1, R):
        d = b[r - 1] - b[r]
        ti += d * (U[r - 1] + U[r]) / 2.0
        ti2 += d * d / 12.0 * (V[r - 1] - V[r])
        w[r - 1] += d / 2.0
        w[r] += d / 2.0
    te = 0.0
    for r in range(R):
        if w[r] != 0.0:
            te += w[r] * w[r] * V[r] / N[r]
    ss, ss_rev = 0.0, 0.0
    for v in fwd:
        ss += v
    for v in rev:
        ss_rev += v
    return dict(log_ratio=np.array(fwd, dtype=np.float64), log_ratio_rev=np.array(rev, dtype=np.float64), ss=ss, ss_err=root_or_nan(vf),
                ss_rev=ss_rev, ss_rev_err=root_or_nan(vr), ti=ti, ti2=ti - ti2, ti_err=root_or_nan(te), beta_min=b[R - 1],
                complete=b[R - 1] == 0.0)


def ladder_evidence(beta, likes, ladder, maxlag=None, engine=None):
    """The log-evidence of every tempering ladder from its recorded rungs (include/bh_engine_chain_ladder_evidence.h).

    A ladder with the betas b_0 > b_1 > ... > b_{R-1} samples, at rung r, the density prior x L^b_r / Z(b_r), Z(b) the integral of
    prior x L^b over the transdimensional prior; Z(1) is the evidence (marginal likelihood) and Z(0) = 1.  Every estimate below is
    log Z(b_0) - log Z(b_min), b_min = b_{R-1}: the log-evidence proper only if the ladder starts at beta = 1 and ends at beta = 0
    (`complete`; whether the sampler behaves at beta = 0 is not this function's matter).  Differences of these numbers between two
    runs on the same data -- with and without a target, under two noise laws, vpvs fixed or free -- are log Bayes factors as far as
    the ladders reach the same b_min.

    beta [T][C] (float64) and likes [T][C] (float32 / float64): the recorded tables, numpy arrays or device tensors, strided views
    of the store included, read where they lie as chain_series_stats reads them; ladder[c]: any integer ids.  The rung series --
    series j = start[k] + r reads chain hold[t][j], the chain of ladder k at rung r, at row t -- come from ladder_evidence_sums;
    their mean, variance and ESS from chain_series_stats(likes, maxlag, sel=hold) and convergence, one series each (maxlag default
    min(T // 2, 1000)).  Returns dict of ids, members, hold, rung_beta, T, maxlag, the sums' arrays [C], and `ladders`: per ladder a
    dict, all float64, D_r = b_{r-1} - b_r, l the rung's likes:
        betas [R];  mean [R] = U_r = E_b_r[log L];  var [R] = V_r = P_0 / T;  tau, ess, rhat [R], ess_truncated [R] of the series
        log_ratio [R-1]      log(Sf_r / T) + D_r mx_r = log mean_t exp(D_r l_r[t])            stepping stones from the hotter rung
        log_ratio_rev [R-1]  -(log(Sr_{r-1} / T) - D_r mn_{r-1}) = -log mean_t exp(-D_r l_{r-1}[t])     ... from the colder rung
        ss, ss_rev           their sums.  The forward estimate is biased low and the reverse high: the two bracket the value.
        ss_err               sqrt(sum_r (T Sf2_r / Sf_r^2 - 1) / ess_r), ss_rev_err likewise: the relative variance of every mean
                             with the rung series' ESS as the number of independent terms -- an approximation
        ti                   sum_r D_r (U_{r-1} + U_r) / 2: thermodynamic integration of dlogZ/db = U, trapezoid
        ti2                  ti - sum_r D_r^2 / 12 (V_{r-1} - V_r): its second-order correction with dU/db = V
        ti_err               sqrt(sum_r w_r^2 V_r / ess_r), w the trapezoid weights
        beta_min, complete = (beta_min == 0.0)
    A ladder of one rung has empty ratios and zeros.  Saved folders hold the cold samples only: nothing of this can be read from
    them.  EngineError: as ladder_holders, and a like that is not finite."""
    eng = _engine(engine)
    out = ladder_evidence_sums(beta, likes, ladder, engine=eng)
    T, Cn = out["T"], int(out["rung_beta"].size)
    L = min(T // 2, 1000) if maxlag is None else int(maxlag)
    tables = chain_series_stats(likes, L, engine=eng, sel=out["hold"])
    conv = convergence(tables, np.arange(Cn))
    out["maxlag"], out["ladders"] = L, []
    start = 0
    for m in out["members"]:
        js = range(start, start + len(m))
        start += len(m)
        stats = dict(mean=[conv[j]["mean"][0, 0] for j in js], var=[tables["p"][j, 0, 0] / T for j in js])
        for k in ("tau", "ess", "rhat", "ess_truncated"):
            stats[k] = [conv[j][k][0] for j in js]
        d = evidence_estimates(T, out["rung_beta"][js.start:js.stop], {k: out[k][js.start:js.stop] for k in EVIDENCE_SUMS},
                               stats["mean"], stats["var"], stats["ess"])
        d["betas"] = out["rung_beta"][js.start:js.stop].copy()
        for k, v in stats.items():
            d[k] = np.array(v, dtype=bool if k == "ess_truncated" else np.float64)
        out["ladders"].append(d)
    return out


def chain_series_stats(values, maxlag, engine=None, sel=None):
    """The sums of the module docstring for every series of a table values[t][c] or values[t][c][q] (float32 / float64; a numpy
    array or a device torch tensor, strided views such as store["misfits"][lo:hi] included -- read where they lie, no copy):
    dict of x0, s1, s1a, s1b, m2a, m2b [C][Q], p [C][Q][maxlag + 1] (float64), T and maxlag.  At most 64 columns go into one
    engine call; wider tables take several.  EngineError: a value that is not finite.
    sel[t][k] (int32, numpy for a numpy table, a device tensor for a device one): the tables of K series instead, series (k, q)
    reading chain sel[t][k] at row t (module docstring) -- the chain axis of every output is the series axis; elements of chains
    not selected at a row are never read.  EngineError: an index outside [0, C)."""
    eng = _engine(engine)
    ptr, mem, stream, elem, shape, strides, keep = _table(values)
    T, Cn = int(shape[0]), int(shape[1])
    if sel is not None:
        return _series_sel(eng, ptr, mem, stream, elem, shape, strides, sel, int(maxlag))
    Q = int(shape[2]) if len(shape) == 3 else 1
    L = int(maxlag)
    if T < 1 or Cn < 1 or Q < 1:
        raise ValueError("an empty table")
    ld_t, ld_c = _lds(shape, strides, Q)
    out = _outputs(Cn, Q, L)
    for q0 in range(0, Q, E.DIAG_MAXCOLS):
        nq = min(E.DIAG_MAXCOLS, Q - q0)
        part = out if nq == Q else _outputs(Cn, nq, L)
        eng._check(eng._L.bh_chain_diag_series(eng._h, mem, stream, elem, T, Cn, nq, ld_t, ld_c, C.c_void_p(ptr.value + q0 * elem), L,
                                               *[E._ptr(part[k]) for k in FIELDS + ("p",)]))
        if part is not out:
            for k in FIELDS + ("p",):
                out[k][:, q0:q0 + nq] = part[k]
    out["T"], out["maxlag"] = T, L
    del keep
    return out


def _series_sel(eng, ptr, mem, stream, elem, shape, strides, sel, L):
    """chain_series_stats of the K series of a selection"""
    T, Cn = int(shape[0]), int(shape[1])
    Q = int(shape[2]) if len(shape) == 3 else 1
    if T < 1 or Cn < 1 or Q < 1:
        raise ValueError("an empty table")
    psel, K, ld_sel, keep = _sel_table(sel, T, Cn, mem)
    ld_t, ld_c = _lds(shape, strides, Q)
    out = _outputs(K, Q, L)
    for q0 in range(0, Q, E.DIAG_MAXCOLS):
        nq = min(E.DIAG_MAXCOLS, Q - q0)
        part = out if nq == Q else _outputs(K, nq, L)
        eng._check(eng._L.bh_chain_diag_series_sel(eng._h, mem, stream, elem, T, Cn, nq, ld_t, ld_c, C.c_void_p(ptr.value + q0 * elem),
                                                   K, psel, ld_sel, L, *[E._ptr(part[k]) for k in FIELDS + ("p",)]))
        if part is not out:
            for k in FIELDS + ("p",):
                out[k][:, q0:q0 + nq] = part[k]
    out["T"], out["maxlag"] = T, L
    del keep
    return out


def chain_model_stats(models, dep, maxlag, engine=None, sel=None):
    """The same for the series derived from model rows models[t][c][2*ML] (the reference's row layout): column q < len(dep) the vs
    at depth dep[q] (the rule of posterior_models), the last column nlayers = n - 1.  The values are formed in the kernel.
    sel: as in chain_series_stats -- series k reads the row of chain sel[t][k]."""
    eng = _engine(engine)
    ptr, mem, stream, elem, shape, strides, keep = _table(models)
    if len(shape) != 3 or shape[2] % 2:
        raise ValueError("models: [T][C][2*ML]")
    T, Cn, ML = int(shape[0]), int(shape[1]), int(shape[2]) // 2
    dep = np.ascontiguousarray(dep, np.float64).reshape(-1)
    D, L = dep.size, int(maxlag)
    if T < 1 or Cn < 1:
        raise ValueError("an empty table")
    ld_t, ld_c = _lds(shape, strides, 2 * ML)
    if sel is not None:
        psel, K, ld_sel, keep_sel = _sel_table(sel, T, Cn, mem)
        out = _outputs(K, D + 1, L)
        eng._check(eng._L.bh_chain_diag_models_sel(eng._h, mem, stream, elem, T, Cn, ML, ld_t, ld_c, ptr, K, psel, ld_sel, D,
                                                   E._ptr(dep), L, *[E._ptr(out[k]) for k in FIELDS + ("p",)]))
        out["T"], out["maxlag"] = T, L
        del keep, keep_sel
        return out
    out = _outputs(Cn, D + 1, L)
    eng._check(eng._L.bh_chain_diag_models(eng._h, mem, stream, elem, T, Cn, ML, ld_t, ld_c, ptr, D, E._ptr(dep), L,
                                           *[E._ptr(out[k]) for k in FIELDS + ("p",)]))
    out["T"], out["maxlag"] = T, L
    del keep
    return out


def chain_medians(likes, engine=None, sel=None):
    """numpy.median of every chain's column of likes[t][c], in the table's dtype: on the GPU for a device tensor (a radix selection
    of the two middle values, include/bh_engine_chain_diag.h), numpy.median itself for a numpy array.
    sel[t][k]: the medians of the K gathered columns likes[t][sel[t][k]] instead (module docstring)."""
    if not _is_tensor(likes):
        a = np.asarray(likes)
        if a.ndim != 2:
            raise ValueError("likes: [T][C]")
        if sel is not None:
            s = np.asarray(sel)
            if s.ndim != 2 or s.shape[0] != a.shape[0] or s.dtype.kind not in "iu":
                raise ValueError("sel: [T][K] integers")
            if s.size and (s.min() < 0 or s.max() >= a.shape[1]):
                raise IndexError("sel: an index outside [0, C)")
            a = np.take_along_axis(a, s.astype(np.int64), 1)
        return np.array([np.median(a[:, c]) for c in range(a.shape[1])], dtype=a.dtype)
    eng = _engine(engine)
    ptr, mem, stream, elem, shape, strides, keep = _table(likes)
    if len(shape) != 2:
        raise ValueError("likes: [T][C]")
    T, Cn = int(shape[0]), int(shape[1])
    ld_t, ld_c = _lds(shape, strides, 1)
    dtype = np.float32 if elem == 4 else np.float64
    if sel is not None:
        psel, K, ld_sel, keep_sel = _sel_table(sel, T, Cn, mem)
        lo, hi = np.zeros(K), np.zeros(K)
        eng._check(eng._L.bh_chain_diag_medians_sel(eng._h, mem, stream, elem, T, Cn, ld_t, ld_c, ptr, K, psel, ld_sel, E._ptr(lo),
                                                    E._ptr(hi)))
        del keep, keep_sel
        return np.array([median_of_middles(lo[k], hi[k], T, dtype) for k in range(K)], dtype=dtype)
    lo, hi = np.zeros(Cn), np.zeros(Cn)
    eng._check(eng._L.bh_chain_diag_medians(eng._h, mem, stream, elem, T, Cn, ld_t, ld_c, ptr, E._ptr(lo), E._ptr(hi)))
    del keep
    return np.array([median_of_middles(lo[c], hi[c], T, dtype) for c in range(Cn)], dtype=dtype)


def outlier_scores(medians):
    """1 - score of every chain against the best one, the three branches of the reference's rule"""
    medians = np.asarray(medians)
    maxlike = np.max(medians)
    if maxlike > 0:
        scores = medians / maxlike
    elif maxlike < 0:
        scores = maxlike / medians
    else:
        scores = np.ones_like(medians)
    return 1 - scores


def outlier_chains(likes, site_of_chain, dev=0.05, engine=None, sel=None):
    """The reference's outlier rule per site.  likes[t][c]: the chains' likelihood series (numpy or device tensor);
    site_of_chain[c]: the chain's site.  Returns (outliers, scores): per site the positions c of its outlier chains (1 - score >
    dev, strictly) and their 1 - score -- what results.get_outliers returns for the site's folder, with file numbers for c.
    sel: the rule on the K gathered series of chain_medians(sel=) instead; site_of_chain then holds one site per series."""
    med = chain_medians(likes, engine=engine, sel=sel)
    site_of_chain = np.asarray(site_of_chain, dtype=np.int64)
    if site_of_chain.shape != med.shape:
        raise ValueError("site_of_chain: one site per chain")
    S = int(site_of_chain.max()) + 1 if site_of_chain.size else 0
    outliers, scores = [], []
    for s in range(S):
        idx = np.flatnonzero(site_of_chain == s)
        if not idx.size:
            outliers.append(idx)
            scores.append(np.zeros(0))
            continue
        sc = outlier_scores(med[idx])
        sel = np.where(sc > dev)
        outliers.append(idx[sel])
        scores.append(sc[sel])
    return outliers, scores


def geyer_tau(rho):
    """(tau, cut, truncated) of an autocorrelation table rho[k], k = 0..L: Geyer's initial monotone sequence (module docstring)"""
    rho = np.asarray(rho, dtype=np.float64)
    npairs = rho.size // 2
    if npairs < 1:
        return np.nan, 0, True
    G = rho[0:2 * npairs:2] + rho[1:2 * npairs:2]
    bad = np.flatnonzero(~(G > 0))
    cut = int(bad[0]) if bad.size else npairs
    G = np.minimum.accumulate(G[:cut])
    return -1.0 + 2.0 * float(np.sum(G)), cut, not bad.size


def _ess_block(p, means, n):
    """(tau, cut, truncated) of the chains with lag sums p[m][L+1] and means[m]"""
    m = p.shape[0]
    Wn = np.mean(p[:, 0]) / (n - 1)
    Bn = np.var(means, ddof=1) if m > 1 else 0.0
    varp = (n - 1) / n * Wn + Bn
    rho = 1.0 - (Wn - np.mean(p, axis=0) / n) / varp
    return geyer_tau(rho)


def convergence(tables, site_of_chain, exclude=()):
    """Split R-hat, ESS and per-chain summaries of every site from the tables of chain_series_stats / chain_model_stats (formulas:
    module docstring).  site_of_chain[c]: the chain's site; exclude: positions c left out (outliers).  Returns one dict per site:
    chains [m] (the kept positions), rhat, ess, tau [Q], cut [Q] (the Geyer cut, in pairs), ess_truncated, constant [Q] (bool),
    mean, std, chain_tau [m][Q]."""
    T, L = int(tables["T"]), int(tables["maxlag"])
    Cn, Q = tables["x0"].shape
    site_of_chain = np.asarray(site_of_chain, dtype=np.int64)
    if site_of_chain.shape != (Cn,):
        raise ValueError("site_of_chain: one site per chain")
    drop = np.zeros(Cn, bool)
    drop[np.asarray(exclude, dtype=np.int64).reshape(-1)] = True
    S = int(site_of_chain.max()) + 1 if Cn else 0
    n, h = T, T // 2
    out = []
    with np.errstate(all="ignore"):
        for s in range(S):
            idx = np.flatnonzero((site_of_chain == s) & ~drop)
            m = idx.size
            r = dict(chains=idx, rhat=np.full(Q, np.nan), ess=np.full(Q, np.nan), tau=np.full(Q, np.nan), cut=np.zeros(Q, np.int64),
                     ess_truncated=np.zeros(Q, bool), constant=np.zeros(Q, bool),
                     mean=np.full((m, Q), np.nan), std=np.full((m, Q), np.nan), chain_tau=np.full((m, Q), np.nan))
            out.append(r)
            if not m:
                continue
            x0, p = tables["x0"][idx], tables["p"][idx]
            r["mean"][:] = x0 + tables["s1"][idx] / n
            if n > 1:
                r["std"][:] = np.sqrt(p[:, :, 0] / (n - 1))
            r["constant"][:] = np.all(p[:, :, 0] == 0, axis=0)
            if n < 4:
                continue
            for q in range(Q):
                if r["constant"][q]:
                    continue
                W = np.mean(np.concatenate((tables["m2a"][idx, q], tables["m2b"][idx, q])) / (h - 1))
                Bh = np.var(np.concatenate((x0[:, q] + tables["s1a"][idx, q] / h, x0[:, q] + tables["s1b"][idx, q] / h)), ddof=1)
                r["rhat"][q] = np.sqrt(((h - 1) / h * W + Bh) / W)
                tau, cut, trunc = _ess_block(p[:, q, :], r["mean"][:, q], n)
                r["tau"][q], r["cut"][q], r["ess_truncated"][q] = tau, cut, trunc
                r["ess"][q] = m * n / max(tau, 1.0 / np.log10(m * n))
                for j in range(m):
                    if p[j, q, 0] > 0:
                        r["chain_tau"][j, q] = _ess_block(p[j:j + 1, q, :], r["mean"][j:j + 1, q], n)[0]
    return out


# ---- rank-normalised diagnostics (module docstring; include/bh_engine_chain_rank.h) ----------------------------------------------
# Wichura (1988), Algorithm AS241, PPND16: the coefficients of the three rational approximations, highest power first
_AS241_A = (2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4,
            1.3731693765509461125e+4, 1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e+0)
_AS241_B = (5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4,
            5.3941960214247511077e+3, 6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0)
_AS241_C = (7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e+0,
            3.64784832476320460504e+0, 5.76949722146069140550e+0, 4.63033784615654529590e+0, 1.42343711074968357734e+0)
_AS241_D = (1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
            6.89767334985100004550e-1, 1.67638483018380384940e+0, 2.05319162663775882187e+0, 1.0)
_AS241_E = (2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2,
            2.96560571828504891230e-1, 1.78482653991729133580e+0, 5.46378491116411436990e+0, 6.65790464350110377720e+0)
_AS241_F = (2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
            1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0)


def _horner(coef, r):
    v = np.full_like(r, coef[0])
    for c in coef[1:]:
        v = v * r + c
    return v


def normal_quantile(p):
    """The quantile function of the standard normal distribution, float64: Wichura's AS241 (PPND16, relative accuracy about 1e-16)
    vectorised in numpy.  The definition of the normal scores of rank_table.  p outside (0, 1): NaN (0 and 1: -inf, +inf)."""
    p = np.asarray(p, dtype=np.float64)
    shape = p.shape
    p = p.reshape(-1)
    x = np.full(p.shape, np.nan)
    with np.errstate(all="ignore"):
        q = p - 0.5
        mid = np.abs(q) <= 0.425
        if mid.any():
            qm = q[mid]
            r = 0.180625 - qm * qm
            x[mid] = _horner(_AS241_A, r) * qm / _horner(_AS241_B, r)
        out = ~mid & (p > 0.0) & (p < 1.0)
        if out.any():
            po, qo = p[out], q[out]
            r = np.sqrt(-np.log(np.where(qo <= 0.0, po, 1.0 - po)))
            near = r <= 5.0
            v = np.empty_like(r)
            rn, rf = r[near] - 1.6, r[~near] - 5.0
            v[near] = _horner(_AS241_C, rn) / _horner(_AS241_D, rn)
            v[~near] = _horner(_AS241_E, rf) / _horner(_AS241_F, rf)
            x[out] = np.where(qo < 0.0, -v, v)
        x[p == 0.0] = -np.inf
        x[p == 1.0] = np.inf
    return x.reshape(shape)


def rank_table(N):
    """zt_N [2N + 1]: the normal score of twice-the-average-rank R2 in a pool of N, normal_quantile((R2/2 - 3/8) / (N + 1/4)).
    R2 of an element lies in [2, 2N]; entries 0 and 1 are NaN and never read."""
    N = int(N)
    if N < 1:
        raise ValueError("a pool of at least one value")
    zt = normal_quantile((np.arange(2 * N + 1, dtype=np.float64) / 2.0 - 0.375) / (N + 0.25))
    zt[:2] = np.nan
    return zt


def _rank_groups(group_of_chain, Cn, T):
    """(group int32 [C], G, zt, zoff int64 [G]) of a grouping: one table per distinct pool size, shared by the groups of that size"""
    group = np.asarray(group_of_chain)
    if group.shape != (Cn,) or group.dtype.kind not in "iu":
        raise ValueError("group_of_chain: one integer per chain, -1 for a chain left out")
    group = np.ascontiguousarray(group, dtype=np.int32)
    G = int(group.max()) + 1 if Cn else 0
    if G < 1:
        raise ValueError("group_of_chain: no chain is kept")
    m = np.bincount(group[group >= 0], minlength=G)
    zoff, parts, at, start = np.zeros(G, np.int64), [], {}, 0
    for g in range(G):
        N = int(m[g]) * T
        if N < 1:
            continue         # (an empty group: the engine refuses it)
        if N not in at:
            at[N] = start
            parts.append(rank_table(N))
            start += 2 * N + 1
        zoff[g] = at[N]
    zt = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(1)
    return group, G, zt, zoff


def _rank_outputs(mem, like, shape, folded, tail):
    """z, zf, tail of a call: device tensors beside a device table, numpy arrays otherwise; and their pointers"""
    T, Cn, Q = shape
    if mem == E.DEVICE:
        import torch
        z = torch.empty((T, Cn, Q), dtype=torch.float64, device=like.device)
        zf = torch.empty((T, Cn, Q), dtype=torch.float64, device=like.device) if folded else None
        tl = torch.empty((T, Cn, 2 * Q), dtype=torch.float32, device=like.device) if tail else None
        return z, zf, tl, [None if a is None else a.data_ptr() for a in (z, zf, tl)]
    z = np.empty((T, Cn, Q))
    zf = np.empty((T, Cn, Q)) if folded else None
    tl = np.empty((T, Cn, 2 * Q), np.float32) if tail else None
    return z, zf, tl, [None if a is None else a.ctypes.data for a in (z, zf, tl)]


def rank_series(values, group_of_chain, engine=None, folded=True, tail=True):
    """The rank transform of every column of a table values[t][c] or values[t][c][q] (float32 / float64, numpy or device tensor,
    strided views read where they lie), pooled over the chains of a group: group_of_chain[c] in 0..G-1 (every group non-empty) is
    the chain's pool -- its site; the chains of a pool need not be adjacent --, -1 leaves the chain out.  Returns (z, zf, tail)
    (module docstring): z, zf float64 shaped as values, tail float32 [T][C][2Q] with (lo, hi) of column q at 2q, 2q + 1; device
    tensors for a device table, numpy arrays for a numpy one; zf / tail None without folded / tail.  The chains left out hold 0.
    EngineError: a value of a kept chain that is not finite, an empty group."""
    eng = _engine(engine)
    ptr, mem, stream, elem, shape, strides, keep = _table(values)
    T, Cn = int(shape[0]), int(shape[1])
    Q = int(shape[2]) if len(shape) == 3 else 1
    if T < 1 or Cn < 1 or Q < 1:
        raise ValueError("an empty table")
    group, G, zt, zoff = _rank_groups(group_of_chain, Cn, T)
    ld_t, ld_c = _lds(shape, strides, Q)
    z, zf, tl, ptrs = _rank_outputs(mem, keep, (T, Cn, Q), folded, tail)
    for q0 in range(0, Q, E.DIAG_MAXCOLS):
        nq = min(E.DIAG_MAXCOLS, Q - q0)
        outs = [None if a is None else C.c_void_p(a + q0 * w) for a, w in zip(ptrs, (8, 8, 8))]
        eng._check(eng._L.bh_chain_rank_series(eng._h, mem, stream, elem, T, Cn, nq, ld_t, ld_c, C.c_void_p(ptr.value + q0 * elem),
                                               G, E._ptr(group), E._ptr(zt), E._ptr(zoff), outs[0], outs[1], outs[2], Cn * Q, Q))
    del keep
    if len(shape) == 2:
        z, zf = z.reshape(T, Cn), (None if zf is None else zf.reshape(T, Cn))
    return z, zf, tl


def rank_models(models, dep, group_of_chain, engine=None, folded=True, tail=True, columns=None):
    """rank_series of the series derived from model rows models[t][c][2*ML] (chain_model_stats: column q < len(dep) the vs at depth
    dep[q], the last column nlayers), the values formed in the kernel.  columns=(q0, nq): those nq of the len(dep) + 1 columns only."""
    eng = _engine(engine)
    ptr, mem, stream, elem, shape, strides, keep = _table(models)
    if len(shape) != 3 or shape[2] % 2:
        raise ValueError("models: [T][C][2*ML]")
    T, Cn, ML = int(shape[0]), int(shape[1]), int(shape[2]) // 2
    dep = np.ascontiguousarray(dep, np.float64).reshape(-1)
    D = dep.size
    q0, nq = (0, D + 1) if columns is None else (int(columns[0]), int(columns[1]))
    if T < 1 or Cn < 1:
        raise ValueError("an empty table")
    if q0 < 0 or nq < 1 or q0 + nq > D + 1:
        raise ValueError("columns: (q0, nq) within the len(dep) + 1 columns")
    group, G, zt, zoff = _rank_groups(group_of_chain, Cn, T)
    ld_t, ld_c = _lds(shape, strides, 2 * ML)
    z, zf, tl, ptrs = _rank_outputs(mem, keep, (T, Cn, nq), folded, tail)
    outs = [None if a is None else C.c_void_p(a) for a in ptrs]
    eng._check(eng._L.bh_chain_rank_models(eng._h, mem, stream, elem, T, Cn, ML, ld_t, ld_c, ptr, D, E._ptr(dep), q0, nq, G,
                                           E._ptr(group), E._ptr(zt), E._ptr(zoff), outs[0], outs[1], outs[2], Cn * nq, nq))
    del keep
    return z, zf, tl


RANK_FIELDS = ("rhat_bulk", "rhat_fold", "rhat", "ess_bulk", "ess_tail_lo", "ess_tail_hi", "ess_tail", "ess_bulk_truncated",
               "ess_tail_lo_truncated", "ess_tail_hi_truncated", "constant_bulk", "constant_fold", "constant_tail_lo",
               "constant_tail_hi")


def rank_summary(conv_z, conv_zf, conv_tail):
    """The dict `rank` of one site from its convergence() dicts of the tables z [Q], zf [Q] and tail [2Q] (pure numpy): chains,
    rhat_bulk, rhat_fold, rhat = the larger (NaN if either is), ess_bulk, ess_tail_lo, ess_tail_hi, ess_tail = the smaller (NaN
    if either is), and of each the flags ess_*_truncated and constant_* [Q]."""
    lo, hi = slice(0, None, 2), slice(1, None, 2)
    return dict(chains=conv_z["chains"], rhat_bulk=conv_z["rhat"], rhat_fold=conv_zf["rhat"],
                rhat=np.maximum(conv_z["rhat"], conv_zf["rhat"]), ess_bulk=conv_z["ess"],
                ess_tail_lo=conv_tail["ess"][lo], ess_tail_hi=conv_tail["ess"][hi],
                ess_tail=np.minimum(conv_tail["ess"][lo], conv_tail["ess"][hi]),
                ess_bulk_truncated=conv_z["ess_truncated"], ess_tail_lo_truncated=conv_tail["ess_truncated"][lo],
                ess_tail_hi_truncated=conv_tail["ess_truncated"][hi], constant_bulk=conv_z["constant"],
                constant_fold=conv_zf["constant"], constant_tail_lo=conv_tail["constant"][lo],
                constant_tail_hi=conv_tail["constant"][hi])


def rank_convergence(values, site_of_chain, maxlag, exclude=(), dep=None, engine=None, budget_bytes=2 << 30):
    """The rank-normalised numbers of every site (module docstring) from a table values[t][c] / values[t][c][q], or -- with dep --
    from model rows (the columns of chain_model_stats): the pools are every site's kept chains (site_of_chain[c], without the
    positions `exclude`), the rank tables go through chain_series_stats and convergence as they are.  The columns are walked in
    chunks so that the rank tables alive at once (24 bytes per element and column) stay under budget_bytes.  One dict per site
    (rank_summary); a site without a kept chain has NaN throughout.  The ESS is on the unsplit chains, as everywhere here."""
    site_of_chain = np.asarray(site_of_chain, dtype=np.int64)
    Cn = int(values.shape[1])
    T = int(values.shape[0])
    if site_of_chain.shape != (Cn,):
        raise ValueError("site_of_chain: one site per chain")
    drop = np.zeros(Cn, bool)
    drop[np.asarray(exclude, dtype=np.int64).reshape(-1)] = True
    kept_sites = np.unique(site_of_chain[~drop])
    group = np.where(drop, -1, np.searchsorted(kept_sites, site_of_chain)).astype(np.int32)
    if dep is not None:
        dep = np.ascontiguousarray(dep, np.float64).reshape(-1)
        Q = dep.size + 1
    else:
        Q = int(values.shape[2]) if len(values.shape) == 3 else 1
    step = int(max(1, min(E.DIAG_MAXCOLS, int(budget_bytes) // max(1, 24 * T * Cn))))
    L = int(maxlag)
    parts = []
    for q0 in range(0, Q, step):
        nq = min(step, Q - q0)
        if dep is not None:
            z, zf, tl = rank_models(values, dep, group, engine=engine, columns=(q0, nq))
        else:
            v = values if len(values.shape) == 2 else values[:, :, q0:q0 + nq]
            z, zf, tl = rank_series(v, group, engine=engine)
        conv = [convergence(chain_series_stats(t, L, engine=engine), site_of_chain, exclude) for t in (z, zf, tl)]
        del z, zf, tl
        parts.append([rank_summary(a, b, c) for a, b, c in zip(*conv)])
    return [{k: (parts[0][s][k] if k == "chains" else np.concatenate([np.atleast_1d(p[s][k]) for p in parts]))
             for k in ("chains",) + RANK_FIELDS} for s in range(len(parts[0]))]


# ---- convergence of structural features (module docstring; include/bh_engine_chain_diag_features.h) ------------------------------

def chain_feature_series(models, features, site_of_series, sel=None, engine=None, nsites=None):
    """The structural features of every recorded model as time-ordered series (bh_chain_diag_features): models[t][c][2*ML], the
    store's rows (float32 / float64, a numpy array or a device tensor, strided views read where they lie); features: the dict of
    posterior.check_features, name -> (kind, z0, z1[, c]) with every number a scalar or one per site -- the same errors, the same
    labels (name, name.depth, name.jump, name.value); site_of_series[k]: the site whose numbers series k takes (nsites: the number
    of sites, default the largest site + 1).  sel[t][k] (ladder_index): K series that read chain sel[t][k] at row t instead of the
    chains' own; rows of chains not selected at a row are never read.
    Returns (value, present, missing, labels): value float64 [T][K][ncols] -- the column's value, +0.0 where the row lacks it --,
    present float32 [T][K][ncols] -- 1 where the row has it --, device tensors for a device table and numpy arrays for a numpy one;
    missing int64 [K][ncols], the rows of series k that lack column q; labels [ncols].  value and present hold, bit for bit, the
    columns posterior_features / posterior_classes(return_columns=True) form for the same rows.
    EngineError: a row that is no model, a value that is not finite, an index outside [0, C)."""
    from .posterior import check_features
    eng = _engine(engine)
    ptr, mem, stream, elem, shape, strides, keep = _table(models)
    if len(shape) != 3 or shape[2] % 2 or shape[2] < 2:
        raise ValueError("models: [T][C][2*ML]")
    T, Cn, ML = int(shape[0]), int(shape[1]), int(shape[2]) // 2
    if T < 1 or Cn < 1:
        raise ValueError("an empty table")
    site = np.asarray(site_of_series)
    if site.ndim != 1 or site.dtype.kind not in "iu" or (site.size and site.min() < 0):
        raise ValueError("site_of_series: one site (an integer >= 0) per series")
    S = (int(site.max()) + 1 if site.size else 0) if nsites is None else int(nsites)
    if site.size and int(site.max()) >= S:
        raise ValueError("site_of_series: a site beyond nsites")
    kinds, par, labels = check_features(features, S)
    ld_t, ld_c = _lds(shape, strides, 2 * ML)
    if sel is not None:
        psel, K, ld_sel, keep_sel = _sel_table(sel, T, Cn, mem)
    else:
        psel, K, ld_sel, keep_sel = None, Cn, 0, None
    if site.shape != (K,):
        raise ValueError("site_of_series: one site per series (%d)" % K)
    site = np.ascontiguousarray(site, dtype=np.int32)
    Q = len(labels)
    if mem == E.DEVICE:
        import torch
        value = torch.empty((T, K, Q), dtype=torch.float64, device=keep.device)
        present = torch.empty((T, K, Q), dtype=torch.float32, device=keep.device)
        pv, pp = C.c_void_p(value.data_ptr()), C.c_void_p(present.data_ptr())
    else:
        value, present = np.empty((T, K, Q)), np.empty((T, K, Q), np.float32)
        pv, pp = E._ptr(value), E._ptr(present)
    missing = np.zeros((K, Q), np.int64)
    eng._check(eng._L.bh_chain_diag_features(eng._h, mem, stream, elem, T, Cn, ML, ld_t, ld_c, ptr, K, psel, ld_sel, S, E._ptr(site),
                                             len(kinds), E._ptr(kinds), E._ptr(par), pv, pp, K * Q, Q, E._ptr(missing)))
    del keep, keep_sel
    return value, present, missing, labels


def _ascending_sum(v):
    """the sum of v [m][Q] over its first axis, row after row in ascending order, starting from 0.0"""
    acc = np.zeros(v.shape[1:])
    for row in v:
        acc = acc + row
    return acc


def pooled_sd(tables, idx):
    """The deviation of every column pooled over the rows of the chains idx (ascending positions), from the tables of
    chain_series_stats -- per chain c the mean mean_c = x0 + S1 / T and the sum of squares P_{c,0} about it, T equal:
        g   = (sum_c mean_c) / m
        sd  = sqrt((sum_c P_{c,0} + T * sum_c (mean_c - g)^2) / (m T - 1))
    every sum over the m chains in ascending order from 0.0.  NaN for m T < 2."""
    T, m = int(tables["T"]), len(idx)
    Q = tables["x0"].shape[1]
    if m * T < 2:
        return np.full(Q, np.nan)
    mean = tables["x0"][idx] + tables["s1"][idx] / T
    g = _ascending_sum(mean) / m
    dev = mean - g
    return np.sqrt((_ascending_sum(tables["p"][idx, :, 0]) + T * _ascending_sum(dev * dev)) / (m * T - 1))


_FEATURE_KEYS = ("rhat", "ess", "tau", "cut", "ess_truncated", "constant", "chain_tau", "chains")


def feature_convergence(value, present, missing, site_of_series, maxlag, exclude=(), engine=None, rank=False, budget_bytes=2 << 30,
                        labels=None):
    """R-hat, ESS and Monte-Carlo standard errors of every feature column of every site, from the tables of chain_feature_series.
    site_of_series[k]: the series' site; exclude: positions k left out (outliers).  The columns are walked in chunks so that the
    tables formed here (8 bytes per element and column, 32 with rank) stay under budget_bytes; every table goes to
    chain_series_stats, convergence and rank_convergence as it is.  One dict per site, all arrays over the Q columns; with the
    site's kept series c = 1..m (ascending), T rows each:
        labels        the columns' labels (where given)
        chains [m]    the kept positions
        missing [m][Q] (int64), complete [Q] = no kept row lacks the column,
        probability [Q] = kept rows with a value / kept rows (m T)
        presence      the convergence() dict of the indicator series `present`, and mcse_probability [Q] = sd(present) /
                      sqrt(ess of present).  A column that is never lacking (or always) has a constant indicator: flagged
                      `constant`, its numbers NaN as for any constant column.
        mean [Q]      the conditional mean  m_q = (sum_c mean_c(value)) / (sum_c mean_c(present)),  mean_c = x0 + S1 / T of
                      chain_series_stats, both sums over the kept series in ascending order from 0.0 (T cancels); NaN where no
                      kept row has the column
        rhat, ess, tau, cut, ess_truncated, constant [Q], chain_tau [m][Q]: the convergence() numbers of the series
                      x = value                         where the column is complete at the site,
                      x = present * (value - m_q)       otherwise -- elementwise in float64 (torch on device tables, numpy on
                      host ones), the subtraction rounded before the product.
                      This is the linearised ratio estimator: the conditional mean is a ratio of two chain averages, mu^ = sum_t
                      I_t v_t / sum_t I_t, and mu^ - mu ~ sum_t I_t (v_t - mu) / (N p): its Monte-Carlo error is that of the
                      mean of x, so R-hat and ESS of x answer for the number a study publishes, where R-hat of the rows that
                      have the feature would drop the time order and ignore how presence itself mixes.
        mcse_mean [Q] = sd(x) / (p_q sqrt(ess)),  p_q = 1 for a complete column and probability[q] otherwise;  sd = pooled_sd,
                      the deviation of x over the kept rows (its docstring states the expression)
    A column no kept row has: probability 0, mean NaN, constant True.  A site without a kept series: NaN throughout.
    rank=True: `rank` = the rank_convergence dict of the value table, with NaN (and False flags) in the columns that are not
    complete at the site, and presence["rank"] = that of `present`."""
    tensor = _is_tensor(value)
    if tensor != _is_tensor(present):
        raise ValueError("value and present: both numpy arrays or both device tensors")
    if len(value.shape) != 3 or tuple(value.shape) != tuple(present.shape):
        raise ValueError("value and present: [T][K][Q] tables of one shape")
    T, K, Q = (int(v) for v in value.shape)
    missing = np.asarray(missing, dtype=np.int64)
    site_of_series = np.asarray(site_of_series, dtype=np.int64)
    if missing.shape != (K, Q) or site_of_series.shape != (K,):
        raise ValueError("missing [K][Q] and site_of_series [K] describe the K series of the tables")
    if labels is not None and len(labels) != Q:
        raise ValueError("labels: one per column")
    drop = np.zeros(K, bool)
    drop[np.asarray(exclude, dtype=np.int64).reshape(-1)] = True
    S = int(site_of_series.max()) + 1 if K else 0
    kept = [np.flatnonzero((site_of_series == s) & ~drop) for s in range(S)]
    complete = np.array([missing[idx].sum(axis=0) == 0 for idx in kept], dtype=bool).reshape(S, Q)
    L = int(maxlag)
    step = int(max(1, min(E.DIAG_MAXCOLS, int(budget_bytes) // max(1, (32 if rank else 8) * T * K))))
    parts = []
    for q0 in range(0, Q, step):
        q1 = min(Q, q0 + step)
        v, p = value[:, :, q0:q1], present[:, :, q0:q1]
        whole = bool(complete[:, q0:q1].all())
        tv = chain_series_stats(v, L if whole else 0, engine=engine)
        tp = chain_series_stats(p, L, engine=engine)
        mean_v, mean_p = tv["x0"] + tv["s1"] / T, tp["x0"] + tp["s1"] / T
        with np.errstate(all="ignore"):
            m = np.array([_ascending_sum(mean_v[idx]) / _ascending_sum(mean_p[idx]) if idx.size else np.full(q1 - q0, np.nan)
                          for idx in kept]).reshape(S, q1 - q0)
        if whole:
            tx = tv
        else:
            # the linearised series of the columns that are not complete at the series' site; value itself elsewhere
            lin = np.zeros((K, q1 - q0), bool)
            shift = np.zeros((K, q1 - q0))
            for s, idx in enumerate(kept):
                lin[site_of_series == s] = ~complete[s, q0:q1]
                shift[site_of_series == s] = np.where(np.isnan(m[s]), 0.0, m[s])
            if tensor:
                import torch
                tl = torch.as_tensor(lin, device=value.device)
                x = torch.where(tl, p.to(torch.float64) * (v - torch.as_tensor(shift, device=value.device)), v)
            else:
                x = np.where(lin, p.astype(np.float64) * (v - shift), v)
            tx = chain_series_stats(x, L, engine=engine)
            del x
        cx, cp = convergence(tx, site_of_series, exclude), convergence(tp, site_of_series, exclude)
        rk = rkp = None
        if rank:
            rk = rank_convergence(v, site_of_series, L, exclude, engine=engine, budget_bytes=budget_bytes)
            rkp = rank_convergence(p, site_of_series, L, exclude, engine=engine, budget_bytes=budget_bytes)
        part = []
        for s, idx in enumerate(kept):
            n = idx.size * T
            r = {k: cx[s][k] for k in _FEATURE_KEYS}
            r["missing"] = missing[idx, q0:q1]
            r["complete"] = complete[s, q0:q1]
            with np.errstate(all="ignore"):
                prob = (n - r["missing"].sum(axis=0)) / float(n) if n else np.full(q1 - q0, np.nan)
                r["probability"] = prob
                r["mean"] = m[s]
                pq = np.where(r["complete"], 1.0, prob)
                r["mcse_mean"] = pooled_sd(tx, idx) / (pq * np.sqrt(r["ess"]))
                r["presence"] = dict(cp[s])
                r["presence"]["mcse_probability"] = pooled_sd(tp, idx) / np.sqrt(cp[s]["ess"])
            if rank:
                gone = ~r["complete"]
                r["rank"] = {}
                for k, a in rk[s].items():
                    if k != "chains":
                        a = a.copy()
                        a[gone] = False if a.dtype == bool else np.nan
                    r["rank"][k] = a
                r["presence"]["rank"] = rkp[s]
            part.append(r)
        parts.append(part)

    out = [_join_columns([p[s] for p in parts]) for s in range(S)]
    if labels is not None:
        for r in out:
            r["labels"] = list(labels)
    return out


def _join_columns(dicts):
    """the dicts of the column chunks of one site as one: `chains` once, a dict key by key, every array along its last axis"""
    if len(dicts) == 1:
        return dicts[0]
    return {k: (v if k == "chains" else _join_columns([d[k] for d in dicts]) if isinstance(v, dict)
                else np.concatenate([d[k] for d in dicts], axis=-1)) for k, v in dicts[0].items()}


def moho_feature(features, moho, mohovs, S):
    """The features dict of a call with moho= added: moho = (lo, hi) or one pair per site is the feature "moho": ("above", lo, hi,
    mohovs) -- the column BH_MOHO_DEPTH of posterior_moho, bit for bit (include/bh_engine_posterior_features.h)."""
    from .posterior import _per_site
    features = dict(features) if features is not None else {}
    if moho is not None:
        if "moho" in features:
            raise ValueError("moho= names its feature 'moho': rename the feature of that name")
        rng = _per_site(moho, S, 2, "moho")
        features["moho"] = ("above", rng[:, 0].copy(), rng[:, 1].copy(), _per_site(mohovs, S, 0, "mohovs"))
    return features


GROUPS = ("likes", "vpvs", "misfits", "noise", "nlayers", "vs")


def diagnose(tables_of, site_of_chain, chain_ids, dev=0.05, dep=None, maxlag=None, exclude_chains=None, engine=None, sel=None,
             rank=False, rank_budget_bytes=2 << 30, features=None, moho=None, mohovs=4.2):
    """Outliers and convergence of every site from the tables of a run: tables_of = dict of likes, vpvs [T][C], misfits [T][C][nt+1],
    noise [T][C][2nt], models [T][C][2*ML] (numpy arrays or device tensors).  chain_ids[c]: the chain's number (what `outliers` and
    exclude_chains hold).  One dict per site: outliers, scores, chain_ids, dep, maxlag, and for every name of GROUPS the dict of
    convergence().  What DeviceChains.diagnostics and results.diagnostics_from_storage share.
    sel[t][k] (ladder_index): the K cold series of a tempered run instead of the chains' own -- site_of_chain and chain_ids then
    describe the K series (the ladders' sites and ids), and everything downstream sees tables of K series.
    rank=True: every group's dict gains the key "rank", the dict of rank_convergence -- the kept chains of a site pooled after the
    outlier rule or exclude_chains has decided who is kept; ValueError with sel (ranks of cold series are not formed).  With the
    default nothing of it runs.
    features (the dict of posterior_features: name -> (kind, z0, z1[, c]), every number a scalar or one per site) and / or
    moho = (lo, hi) or one pair per site, with mohovs (the feature "moho": ("above", lo, hi, mohovs), posterior_moho's depth column
    bit for bit): every site's dict gains the key "features", the dict of feature_convergence -- R-hat, ESS and the Monte-Carlo
    standard error of every feature column over the site's kept chains, `chains` as chain numbers.  The series are formed on the
    GPU from the model rows where they lie (chain_feature_series; with sel the cold series are read in place).  With the defaults
    nothing of it runs and every dict has the keys it has without."""
    if rank and sel is not None:
        raise ValueError("rank=True with sel=: the ranks of the cold series of tempered runs are not formed")
    chain_ids = np.asarray(chain_ids, dtype=np.int64)
    site_of_chain = np.asarray(site_of_chain, dtype=np.int64)
    T = int(tables_of["likes"].shape[0])
    dep = np.linspace(0, 100, 41) if dep is None else np.asarray(dep, dtype=np.float64)
    L = min(T // 2, 1000) if maxlag is None else int(maxlag)
    outl, scores = outlier_chains(tables_of["likes"], site_of_chain, dev=dev, engine=engine, sel=sel)
    if exclude_chains is None:
        exclude = np.concatenate(outl) if outl else np.zeros(0, np.int64)
    else:
        ex = np.atleast_1d(np.asarray(exclude_chains, dtype=np.int64))
        pos = {int(c): i for i, c in enumerate(chain_ids)}
        if any(int(c) not in pos for c in ex):
            raise IndexError("exclude_chains: a chain number that is not one of the run's")
        exclude = np.array([pos[int(c)] for c in ex], dtype=np.int64)
    S = int(site_of_chain.max()) + 1
    out = [dict(outliers=chain_ids[outl[s]], scores=scores[s], chain_ids=chain_ids[site_of_chain == s], dep=dep, maxlag=L)
           for s in range(S)]
    conv = {k: convergence(chain_series_stats(tables_of[k], L, engine=engine, sel=sel), site_of_chain, exclude)
            for k in ("likes", "vpvs", "misfits", "noise")}
    mt = chain_model_stats(tables_of["models"], dep, L, engine=engine, sel=sel)
    D = dep.size
    both = convergence(mt, site_of_chain, exclude)
    for s in range(S):
        for k in conv:
            out[s][k] = conv[k][s]
        out[s]["vs"] = {k: (v if k == "chains" else v[..., :D]) for k, v in both[s].items()}
        out[s]["nlayers"] = {k: (v if k == "chains" else v[..., D]) for k, v in both[s].items()}
        for k in GROUPS:
            out[s][k]["chains"] = chain_ids[out[s][k]["chains"]]
    if features is not None or moho is not None:
        fts = moho_feature(features, moho, mohovs, S)
        value, present, missing, labels = chain_feature_series(tables_of["models"], fts, site_of_chain, sel=sel, engine=engine, nsites=S)
        fc = feature_convergence(value, present, missing, site_of_chain, L, exclude, engine=engine, rank=rank,
                                 budget_bytes=rank_budget_bytes, labels=labels)
        del value, present
        for s in range(S):
            out[s]["features"] = fc[s]
            for d in (fc[s], fc[s]["presence"]) + ((fc[s]["rank"], fc[s]["presence"]["rank"]) if rank else ()):
                d["chains"] = chain_ids[d["chains"]]
    if rank:
        rk = {k: rank_convergence(tables_of[k], site_of_chain, L, exclude, engine=engine, budget_bytes=rank_budget_bytes)
              for k in ("likes", "vpvs", "misfits", "noise")}
        rboth = rank_convergence(tables_of["models"], site_of_chain, L, exclude, dep=dep, engine=engine, budget_bytes=rank_budget_bytes)
        for s in range(S):
            for k in rk:
                out[s][k]["rank"] = rk[k][s]
            out[s]["vs"]["rank"] = {k: (v if k == "chains" else v[..., :D]) for k, v in rboth[s].items()}
            out[s]["nlayers"]["rank"] = {k: (v if k == "chains" else v[..., D]) for k, v in rboth[s].items()}
            for k in GROUPS:
                out[s][k]["rank"]["chains"] = chain_ids[out[s][k]["rank"]["chains"]]
    return out


def stack_chain_files(datapath):
    """the c???_p2{likes,vpvs,misfits,noise,models}.npy of a folder as [T][C][..] tables, and the chains' file numbers"""
    from .results import _chainfiles, _chainidx
    files = _chainfiles(datapath, 2, "likes")
    if not files:
        raise IOError("%s: no c???_p2likes.npy" % datapath)
    ids = np.array([_chainidx(f) for f in files], dtype=np.int64)
    tabs = {}
    for k in ("likes", "vpvs", "misfits", "noise", "models"):
        cols = [np.load(f.replace("likes.npy", k + ".npy")) for f in files]
        if len(set(len(c) for c in cols)) != 1:
            raise ValueError("%s: chains of unequal length (%s)" % (datapath, k))
        a = np.stack(cols, axis=1)
        if k in ("likes", "vpvs"):
            a = a.reshape(a.shape[0], a.shape[1])
        elif a.ndim == 2:
            a = a[:, :, None]
        tabs[k] = np.ascontiguousarray(a)
    return tabs, ids
