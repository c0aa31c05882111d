"""The restatement of the ladder index (tests/ladder_ref.py) against parallel.cold_samples' pick and hand-worked tables.  The GPU
tests hold bayhunter_amd.diagnostics.ladder_index to this restatement (tests/test_gpu_chain_diag_ladders.py)."""
import numpy as np
import pytest

import ladder_ref as LR
from bayhunter_amd.parallel import cold_samples

B3 = [1.0, 0.5, 0.1]      # a 3-rung ladder: cold, mid, hot


def cold_pick(beta, ladder):
    """the chain cold_samples picks per (row, ladder): its gather applied to the chains' own numbers"""
    T, C = beta.shape
    ids, out = cold_samples(dict(beta=beta, chain=np.tile(np.arange(C), (T, 1))), ladder)
    return ids, out["chain"]


@pytest.mark.parametrize("tie", [False, True])
@pytest.mark.parametrize("T,ladder", [(1, [0, 0, 0]), (7, [0, 1, 0, 1, 2, 0, 1]), (33, [5, 5, 5, 5, 2, 2, 9]),
                                      (12, list(np.repeat(np.arange(3), 4))), (5, [3] * 64 + [1] * 5 + [7])])
def test_sel_is_the_pick_of_cold_samples(T, ladder, tie):
    rs = np.random.RandomState(T + len(ladder))
    beta = LR.permuted_betas(rs, T, ladder, tie=tie)
    r = LR.ladder_index(beta, ladder)
    ids, pick = cold_pick(beta, np.asarray(ladder))
    assert np.array_equal(r["ids"], ids) and np.array_equal(r["sel"], pick)
    mask = np.zeros(beta.shape, bool)
    mask[np.arange(T)[:, None], r["sel"]] = True
    assert np.array_equal(mask, LR.cold_mask(beta, ladder))
    assert np.all(r["occupancy"].sum(axis=1) == T) and np.all(r["rung"][np.arange(T)[:, None], r["sel"]] == 0)
    sizes = np.array([len(m) for m in r["members"]])
    assert r["occupancy"].shape == (len(ladder), sizes.max())
    if not tie:     # a permutation of distinct betas: every rung of a ladder is held by exactly one chain at every row
        for m in r["members"]:
            assert np.all(np.sort(r["rung"][:, m], axis=1) == np.arange(len(m)))
            assert np.all(r["hot"][:, m].sum(axis=1) == (1 if len(m) > 1 else 0))


def test_a_chain_that_goes_cold_hot_cold_mid_hot_cold_makes_two_trips():
    # chain 0: cold, hot, cold, mid, hot, cold; chains 1 and 2 take what is left
    c0 = [0, 2, 0, 1, 2, 0]
    rest = {0: (1, 2), 1: (0, 2), 2: (0, 1)}
    beta = np.array([[B3[r], B3[rest[r][0]], B3[rest[r][1]]] for r in c0])
    r = LR.ladder_index(beta, [4, 4, 4])
    assert list(r["rung"][:, 0]) == c0 and list(r["hot"][:, 0]) == [False, True, False, False, True, False]
    assert r["round_trips"][0] == 2 and list(r["occupancy"][0]) == [3, 1, 2]
    # chain 1 holds rungs 1, 0, 1, 0, 0, 1: cold twice in a row, never hot -- no trip; chain 2: 2, 1, 2, 2, 1, 2 -- never cold
    assert list(r["rung"][:, 1]) == [1, 0, 1, 0, 0, 1] and list(r["round_trips"]) == [2, 0, 0]
    assert list(r["sel"][:, 0]) == [0, 1, 0, 1, 1, 0] and list(r["moves"]) == [4] and list(r["ids"]) == [4]
    # a hot row before any cold row does not open a trip
    late = LR.ladder_index(beta[1:], [4, 4, 4])
    assert late["round_trips"][0] == 1


def test_a_one_chain_ladder_is_always_cold():
    beta = np.array([[1.0, 0.3], [0.25, 1.0], [1.0, 1.0]])
    r = LR.ladder_index(beta, [0, 1])
    assert not r["rung"].any() and not r["hot"].any() and list(r["round_trips"]) == [0, 0] and list(r["moves"]) == [0, 0]
    assert np.array_equal(r["sel"], [[0, 1]] * 3) and np.array_equal(r["occupancy"], [[3], [3]])


def test_a_tie_at_beta_one_goes_to_the_first_chain_and_both_are_cold():
    beta = np.array([[0.2, 1.0, 1.0], [1.0, 0.2, 1.0], [0.2, 0.2, 1.0]])
    r = LR.ladder_index(beta, [0, 0, 0])
    assert list(r["sel"][:, 0]) == [1, 0, 2]
    assert np.array_equal(r["rung"], [[2, 0, 0], [0, 2, 0], [1, 1, 0]])
    assert np.array_equal(r["hot"], [[True, False, False], [False, True, False], [True, True, False]])
    ids, pick = cold_pick(beta, np.zeros(3, int))
    assert np.array_equal(pick, r["sel"])


def test_one_row():
    r = LR.ladder_index(np.array([[0.5, 1.0, 1.0, 0.1]]), [0, 0, 1, 1])
    assert np.array_equal(r["sel"], [[1, 2]]) and np.array_equal(r["rung"], [[1, 0, 0, 1]]) and not r["moves"].any()
    assert not r["round_trips"].any() and np.array_equal(r["occupancy"], [[0, 1], [1, 0], [1, 0], [0, 1]])
