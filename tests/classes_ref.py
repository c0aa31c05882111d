"""A plain restatement of the class rule (include/bh_engine_posterior_classes.h, bayhunter_amd/posterior.py: posterior_classes),
written from the rule: one Python loop per row and term, float64 comparisons, nothing vectorised, nothing of the package imported.
It takes the per-row columns -- what tests/features_ref.py and tests/moho_ref.py give, or what the caller attached -- and gives
every row's class and the counts.  tests/test_classes_ref.py holds it to hand-made rows; the GPU tests use it as their oracle.

The rule.  K classes, T terms; term t = (k, label, op, lo [S], hi [S]) belongs to class k, the terms ascending in k.  With v the
row's value in the column `label` and s the row's site the term holds where
  op "in":    v is not NaN and lo[s] <= v < hi[s];      op "has":   v is not NaN;      op "lacks": v is NaN.
A class holds where all of its terms hold (a class without a term: always).  The row's class is the smallest k that holds, -1
where none does and for a row that is not loaded.
"""
import numpy as np

OPS = ("in", "has", "lacks")   # BH_CLASS_IN, BH_CLASS_HAS, BH_CLASS_LACKS


def term_holds(v, op, lo, hi):
    v = np.float64(v)
    isnan = bool(v != v)
    if op == "in":
        return (not isnan) and bool(np.float64(lo) <= v) and bool(v < np.float64(hi))
    if op == "has":
        return not isnan
    if op == "lacks":
        return isnan
    raise ValueError("unknown op %r" % (op,))


def classify(columns, terms, K, site, loaded, S):
    """(cls int32 [N], counts int64 [S][K + 1]).  columns: label -> float64 [N] by input row; terms: a list of (k, label, op, lo, hi)
    with lo, hi one number or [S]; site [N] (None: every row is site 0); loaded bool [N]: the rows the load kept."""
    loaded = np.asarray(loaded, bool)
    N = len(loaded)
    site = np.zeros(N, np.int64) if site is None else np.asarray(site)
    ks = [t[0] for t in terms]
    if ks != sorted(ks) or any(not 0 <= k < K for k in ks):
        raise ValueError("the terms must ascend in their class, inside [0, K)")
    cls = np.full(N, -1, np.int32)
    counts = np.zeros((S, K + 1), np.int64)
    for r in range(N):
        if not loaded[r]:
            continue
        s = int(site[r])
        got = -1
        for k in range(K):
            holds = True
            for (tk, label, op, lo, hi) in terms:
                if tk != k:
                    continue
                lo_s = lo if np.ndim(lo) == 0 else lo[s]
                hi_s = hi if np.ndim(hi) == 0 else hi[s]
                if not term_holds(columns[label][r], op, lo_s, hi_s):
                    holds = False
                    break
            if holds:
                got = k
                break
        cls[r] = got
        counts[s, got if got >= 0 else K] += 1
    return cls, counts


def rule_terms(classes):
    """the user's ordered dict name -> [(label, lo, hi) | (label, "has") | (label, "lacks")] as (names, the terms of classify)"""
    names, terms = [], []
    for k, (name, ts) in enumerate(classes.items()):
        names.append(name)
        for t in ts:
            if len(t) == 3:
                terms.append((k, t[0], "in", t[1], t[2]))
            else:
                terms.append((k, t[0], t[1], -np.inf, np.inf))
    return names, terms
