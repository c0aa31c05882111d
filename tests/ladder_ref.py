"""A plain restatement of the ladder index of tempered runs (include/bh_engine_chain_diag_ladders.h, bayhunter_amd.diagnostics.ladder_index)
that imports nothing of the package: loops over rows and chains, integers throughout.

beta[t][c]: the recorded betas; ladder[c]: any integer ids.  With M(c) the chains of c's ladder:
    rung[t][c]      = #{c' in M(c) : beta[t][c'] > beta[t][c]}      (0 is cold; ties share a rung)
    sel[t][k]       = min{c in ladder k : rung[t][c] == 0}           (k: the position of the ladder's id among the sorted ids)
    hot[t][c]       : no chain of M(c) has a smaller beta and rung[t][c] > 0
    occupancy[c][r] = #{t : rung[t][c] == r},  r < R = the largest ladder's size
    round_trips[c]  : walk t ascending with a state in {none, cold seen, hot seen after cold}; a cold row in the third state counts
                      one trip; every cold row sets "cold seen"; a hot row in "cold seen" sets the third state
    moves[k]        = #{t >= 1 : sel[t][k] != sel[t-1][k]}
"""
import numpy as np


def ladder_index(beta, ladder):
    beta = np.asarray(beta, dtype=np.float64)
    T, C = beta.shape
    ladder = [int(v) for v in np.asarray(ladder).reshape(-1)]
    assert len(ladder) == C
    ids = sorted(set(ladder))
    members = [[c for c in range(C) if ladder[c] == lid] for lid in ids]
    of = {c: k for k, m in enumerate(members) for c in m}
    K, R = len(ids), max(len(m) for m in members)
    rung = np.zeros((T, C), np.int32)
    hot = np.zeros((T, C), bool)
    sel = np.zeros((T, K), np.int32)
    for t in range(T):
        for c in range(C):
            above = below = 0
            for o in members[of[c]]:
                if beta[t, o] > beta[t, c]:
                    above += 1
                if beta[t, o] < beta[t, c]:
                    below += 1
            rung[t, c] = above
            hot[t, c] = below == 0 and above > 0
        for k in range(K):
            sel[t, k] = min(c for c in members[k] if rung[t, c] == 0)
    occupancy = np.zeros((C, R), np.int64)
    trips = np.zeros(C, np.int64)
    for c in range(C):
        state = 0
        for t in range(T):
            occupancy[c, rung[t, c]] += 1
            if rung[t, c] == 0:
                if state == 2:
                    trips[c] += 1
                state = 1
            elif hot[t, c] and state == 1:
                state = 2
    moves = np.zeros(K, np.int64)
    for k in range(K):
        for t in range(1, T):
            if sel[t, k] != sel[t - 1, k]:
                moves[k] += 1
    return dict(ids=np.array(ids, dtype=np.int64), members=[np.array(m, dtype=np.int64) for m in members], sel=sel, rung=rung, hot=hot,
                occupancy=occupancy, round_trips=trips, moves=moves)


def cold_mask(beta, ladder):
    """bool [T][C]: the rule of DeviceChains._cold_mask -- per row and ladder the first chain that holds the ladder's largest beta"""
    beta = np.asarray(beta, dtype=np.float64)
    ladder = np.asarray(ladder).reshape(-1)
    T, C = beta.shape
    mask = np.zeros((T, C), bool)
    for t in range(T):
        for lid in set(ladder.tolist()):
            top, first = -np.inf, -1
            for c in range(C):
                if ladder[c] == lid and beta[t, c] > top:
                    top, first = beta[t, c], c
            mask[t, first] = True
    return mask


def permuted_betas(rs, T, ladder, tie=False):
    """[T][C]: every row a random permutation of every ladder's geometric temperatures (largest beta 1); tie: two chains of every
    ladder of three or more hold beta 1"""
    ladder = np.asarray(ladder).reshape(-1)
    beta = np.zeros((T, ladder.size))
    for lid in np.unique(ladder):
        idx = np.flatnonzero(ladder == lid)
        b = 1.0 / np.geomspace(1.0, 20.0, idx.size) if idx.size > 1 else np.ones(1)
        if tie and idx.size >= 3:
            b[1] = 1.0
            b[-1] = b[-2]         # ... and two share the smallest
        for t in range(T):
            beta[t, idx] = rs.permutation(b)
    return beta
