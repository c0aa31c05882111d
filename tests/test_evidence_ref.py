"""The evidence estimates of tempered runs without a GPU: the restatement tests/evidence_ref.py against the ladder index's restatement,
against a toy computed by hand, and on a ladder whose evidence is known in closed form."""
import math

import numpy as np
import pytest

import evidence_ref as V
import ladder_ref as LR

LADDERS = {"one of 1": [3], "2, 5, 3 interleaved": [0, 1, 2, 1, 0, 1, 2, 1, 2, 1], "one of 64": [9] * 64}


@pytest.mark.parametrize("which", sorted(LADDERS))
@pytest.mark.parametrize("T", [1, 17, 40])
def test_holders_agree_with_the_ladder_index(which, T):
    ladder = LADDERS[which]
    beta = LR.permuted_betas(np.random.RandomState(T), T, ladder)
    want = LR.ladder_index(beta, ladder)
    ids, members, hold, rb = V.holders(beta, ladder)
    assert np.array_equal(ids, want["ids"]) and all(np.array_equal(a, b) for a, b in zip(members, want["members"]))
    start = np.cumsum([0] + [len(m) for m in members])
    for k, m in enumerate(members):
        for t in range(T):
            for r in range(len(m)):
                c = hold[t, start[k] + r]
                assert c in m and want["rung"][t, c] == r and beta[t, c] == rb[start[k] + r]
        assert np.all(np.diff(rb[start[k]:start[k + 1]]) < 0)
        assert np.array_equal(hold[:, start[k]], want["sel"][:, k])          # rung 0 is the cold series' selection


def test_refusals_of_the_restatement():
    ladder = [0, 0, 0, 1, 1]
    beta = LR.permuted_betas(np.random.RandomState(1), 6, ladder)
    likes = -np.arange(30.0).reshape(6, 5)
    V.sums(beta, likes, ladder)
    b = beta.copy()
    b[2, 1] = b[2, 0]
    with pytest.raises(ValueError, match="tied betas"):
        V.holders(b, ladder)
    b = beta.copy()
    b[5, :3] *= 0.5
    with pytest.raises(ValueError, match="change within the rows"):
        V.holders(b, ladder)
    for bad in (np.nan, np.inf):
        b = beta.copy()
        b[0, 4] = bad
        with pytest.raises(ValueError, match="beta is not finite"):
            V.holders(b, ladder)
        l = likes.copy()
        l[3, 3] = bad
        with pytest.raises(ValueError, match="like is not finite"):
            V.sums(beta, l, ladder)


def test_stepping_stones_of_a_two_rung_toy_by_hand():
    """betas 1 and 0.5 swapping between two chains over three rows; every number written out"""
    beta = np.array([[1.0, 0.5], [0.5, 1.0], [1.0, 0.5]])
    likes = np.array([[-2.0, -8.0], [-6.0, -1.0], [-3.0, -4.0]])
    cold, hot = [-2.0, -1.0, -3.0], [-8.0, -6.0, -4.0]         # the series of rung 0 and rung 1
    s = V.sums(beta, likes, [0, 0])
    assert np.array_equal(s["hold"], [[0, 1], [1, 0], [0, 1]]) and list(s["rung_beta"]) == [1.0, 0.5]
    assert list(s["mx"]) == [-1.0, -4.0] and list(s["mn"]) == [-3.0, -8.0]
    # forward, from the hot rung with step 0.5: exp(0.5 (l + 4)) = e^-2, e^-1, 1; the cold rung's forward step is 0: T
    assert s["sf"][1] == (math.exp(-2.0) + math.exp(-1.0)) + 1.0 and s["sf"][0] == 3.0 and s["sf2"][0] == 3.0
    assert s["sf2"][1] == (math.exp(-2.0) * math.exp(-2.0) + math.exp(-1.0) * math.exp(-1.0)) + 1.0
    # reverse, from the cold rung: exp(-0.5 (l + 3)) = e^-0.5, e^-1, 1; the hot rung's reverse step is 0
    assert s["sr"][0] == (math.exp(-0.5) + math.exp(-1.0)) + 1.0 and s["sr"][1] == 3.0 and s["sr2"][1] == 3.0
    d = V.estimates(3, s["rung_beta"], s, [-2.0, -6.0], [2.0 / 3.0, 8.0 / 3.0], [3.0, 3.0])
    # the identity: log mean exp(D l) of the hot series, and minus log mean exp(-D l) of the cold one
    want = math.log(sum(math.exp(0.5 * v) for v in hot) / 3.0)
    want_rev = -math.log(sum(math.exp(-0.5 * v) for v in cold) / 3.0)
    assert abs(d["log_ratio"][0] - want) < 1e-14 and abs(d["log_ratio_rev"][0] - want_rev) < 1e-14
    assert d["ss"] == d["log_ratio"][0] and d["ss_rev"] == d["log_ratio_rev"][0] and d["ss_rev"] > d["ss"]
    assert d["ti"] == 0.5 * (-2.0 + -6.0) / 2.0 and abs(d["ti2"] - (d["ti"] - 0.25 / 12.0 * (2.0 / 3.0 - 8.0 / 3.0))) < 1e-15
    assert abs(d["ti_err"] - math.sqrt(0.0625 * (2.0 / 3.0) / 3.0 + 0.0625 * (8.0 / 3.0) / 3.0)) < 1e-15
    assert d["beta_min"] == 0.5 and not d["complete"]


def test_dropped_terms_small_steps_and_constant_series():
    """a term at or below -512 is exactly 0; a step of 2^-40 on a flat series takes exp's 1 + x branch; a step of 0 returns T and T"""
    T = 35
    rs = np.random.RandomState(2)
    ladder = [0, 0, 0]
    beta = np.tile([1.0, 1.0 - 2.0 ** -40, 0.25], (T, 1))
    likes = -5.0 - rs.uniform(0, 5995.0, size=(T, 3))
    likes[:, 1] = -100.0 - 2.0 ** -20 * np.arange(T)
    s = V.sums(beta, likes, ladder)
    assert s["sf"][0] == T and s["sf2"][0] == T and s["sr"][2] == T and s["sr2"][2] == T
    wf, _ = V.series_terms([float(v) for v in likes[:, 2]], s["mx"][2], s["mn"][2], 1.0 - 2.0 ** -40 - 0.25, 0.0)
    assert 0.0 in wf and 1.0 in wf and s["sf"][2] >= 1.0
    a = [2.0 ** -40 * (float(v) - s["mx"][1]) for v in likes[:, 1]]
    assert any(0 < -v < 2.0 ** -54 for v in a) and all(V.term(v) == 1.0 + v for v in a if -v < 2.0 ** -54)


def test_the_analytic_ladder():
    """log Z = -2 log 101 in closed form; the three estimates within 4 of their own reported errors (a condition: a numpy version of
    the formulas with plain means and T for the ESS stayed inside it for seeds 0-39, at worst 2.0 / 2.3 / 2.4 errors).  The plain
    trapezoid is off by about -0.3 on this ladder: held to the restatement's own formula only."""
    beta, likes, ladder = V.analytic_ladder(0)
    assert likes.dtype == np.float32 and beta.shape == (2048, 12)
    ev = V.evidence(beta, likes, ladder, maxlag=64)
    d = ev["ladders"][0]
    assert list(d["betas"]) == list(V.ANALYTIC_BETAS) and d["complete"] and d["beta_min"] == 0.0
    for name, value, err, dist in V.within_errors(d):
        print("%-7s %.6f +- %.6f: %.2f errors from %.6f" % (name, value, err, dist, V.ANALYTIC_LOGZ))
        assert err > 0 and dist <= 4.0, (name, value, err, dist)
    assert d["ss"] < d["ss_rev"] + 6.0 * (d["ss_err"] + d["ss_rev_err"])
    D = -np.diff(d["betas"])
    assert abs(d["ti"] - float(np.sum(D * (d["mean"][:-1] + d["mean"][1:]) / 2.0))) < 1e-12
    assert np.all(d["ess"] <= 2048 * math.log10(2048)) and np.all(d["ess"] > 500)
