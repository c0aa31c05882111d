"""The round decisions of the trial-per-lane dispersion kernel keep the SEARCH (csrc/swd_lean.hip, the round loop outside the
secular evaluations): the fused Rayleigh + Love call against tests/golden/lean_decision_bits.npz, which
tools/record_lean_decision_bits.py recorded -- inputs and outputs together -- with the library of the commit before the decision
stage was rewritten.  Velocities are compared as bits, with them the failure flags, the guard's counts and the guarded models per
target, and -- from the counting build -- the counters that are functions of the search: evaluations, layer steps, the sum and
the maximum of the wavefronts' rounds per wave type (in the calls without a guarded model: the re-run launch of the others
writes its clocks over those words; at the c2 shape the maximum only: the sum hangs on which models share a wavefront, which
the ordering launch does not decide the same way twice), the guard's reasons.  The calls are the recorder's own (compute(), imported
from the tool); nothing is drawn here but the c2 shape's models, whose digest the golden keeps."""
import os
import sys

import numpy as np
import pytest

from conftest import REPO, golden

sys.path.insert(0, os.path.join(REPO, "tools"))
import record_lean_decision_bits as T  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return {k: v for k, v in golden("lean_decision_bits.npz").items()}


@pytest.fixture(scope="module")
def got(engine, gold):
    """every recorded call once, shared by the tests below (the search and arithmetic it selects are the engine's defaults; the
    suite's autouse fixture puts back what it had set)"""
    search, arith = engine.swd_search(), engine.swd_arith()
    out = T.compute(engine, gold)
    engine.set_swd_search(search)
    engine.set_swd_arith(arith)
    return out


def _same(got, gold, key):
    a, b = got[key], gold[key]
    assert a.dtype == b.dtype and a.shape == b.shape, (key, a.dtype, b.dtype, a.shape, b.shape)
    if key.endswith("_words") and gold[key[:-6] + "_guard"].any():
        # A call with guarded models ends with the re-run launch, whose kernel adds its phase CLOCKS to words 1 ... 6: there the
        # rounds' sums and maxima are not to be had (two runs of one library differ in them); the other words hold.
        keep = [i for i, w in enumerate(T.WORDS) if w not in (1, 3, 4, 6)]
        a, b = a[keep], b[keep]
    elif key.startswith("c2_") and key.endswith("_words"):
        # At this shape the models are put in order by a parallel launch before the search (which four models share a wavefront
        # hangs on the order of its atomics), and a wavefront's rounds are those of its longest model: the SUM of the rounds moves
        # by a few in 54 000 between two runs of one library (54 037 and 54 044 with the library the golden was recorded with,
        # profiles/lean_decision_parent_rounds.txt); the longest wavefront's rounds and every other word hold.
        keep = [i for i, w in enumerate(T.WORDS) if w not in (1, 4)]
        a, b = a[keep], b[keep]
    if a.dtype == np.float32:  # bits; where the golden holds NaN the value must be NaN
        bad = np.argwhere((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b)))
        assert bad.shape[0] == 0, (key, bad[:8], a[tuple(bad[0])], b[tuple(bad[0])])
    else:
        assert np.array_equal(a, b), (key, a, b)


def _case(got, gold, tag):
    keys = sorted(k for k in gold if k.startswith(tag + "_"))
    assert keys and keys == sorted(k for k in got if k.startswith(tag + "_")), (tag, keys)
    for k in keys:
        _same(got, gold, k)
    return keys


def test_the_golden_holds_every_case(gold):
    tags = ["%s_t16_%s" % (p, b) for p in ("synth", "prior", "odd", "odd1", "c2") for b in ("run", "cnt")] + ["prior_t%d_cnt" % t for t in T.OTHER_TRIALS]
    for t in tags:
        assert t + "_err" in gold and t + "_guard" in gold and t + "_glist_r" in gold and t + "_glist_l" in gold, t
        assert (t + "_words" in gold) == t.endswith("_cnt"), t
        assert (t + "_vel_r" in gold) != (t + "_vel_r_sha" in gold), t
    assert gold["synth_nlay"].size == 96 and gold["prior_nlay"].size == 256 and gold["odd_nlay"].size == 13
    assert gold["periods"].size == 30 and gold["one_period"].size == 1
    assert gold["prior_nlay"].min() >= 2 and gold["prior_nlay"].max() <= 21
    assert gold["odd_model"][2, 0, 1] == 0.0 and np.isnan(gold["odd_model"][2, 3, 2])


@pytest.mark.parametrize("pop", ["synth", "prior", "odd", "odd1"])
def test_fused_call_16_trials(got, gold, pop):
    """velocities as bits, flags, the guard's counts and lists; the counting build: the same, and the search's counters"""
    for build in ("run", "cnt"):
        keys = _case(got, gold, "%s_t16_%s" % (pop, build))
        assert int(gold["%s_t16_%s_sched" % (pop, build)][0]) == 0
        print("%s %s: %d arrays equal; failed %d, guard %s" % (pop, build, len(keys), int((gold["%s_t16_%s_err" % (pop, build)] != 0).sum()),
                                                              gold["%s_t16_%s_guard" % (pop, build)].tolist()))
    for k in ("vel_r", "vel_l", "err", "guard", "glist_r", "glist_l"):  # counting or not: one search
        a, b = got["%s_t16_run_%s" % (pop, k)], got["%s_t16_cnt_%s" % (pop, k)]
        assert np.array_equal(a, b, equal_nan=(a.dtype == np.float32)), (pop, k)


def test_odd_batch_is_what_it_claims(gold):
    """the water-layer model is guarded on both targets, the model with a value that is no number fails, their neighbours do not"""
    for tag in ("odd_t16_run", "odd1_t16_run"):
        assert 1 in gold[tag + "_glist_r"] and 1 in gold[tag + "_glist_l"], tag
        assert gold[tag + "_err"][2] != 0 and gold[tag + "_err"][0] == 0 and gold[tag + "_err"][3] == 0 and gold[tag + "_err"][12] == 0, tag


@pytest.mark.parametrize("trials", T.OTHER_TRIALS)
def test_counting_build_other_trial_counts(got, gold, trials):
    _case(got, gold, "prior_t%d_cnt" % trials)
    print("prior, %d trials: words %s = %s" % (trials, list(T.WORDS), gold["prior_t%d_cnt_words" % trials].tolist()))


def test_c2_shape_once(got, gold):
    """4096 models, both targets: the launch with the priority schedule and the pairing of the SIMDs' wavefronts"""
    for build in ("run", "cnt"):
        tag = "c2_t16_%s" % build
        _case(got, gold, tag)
        assert int(gold[tag + "_sched"][0]) == 1 and int(got[tag + "_sched"][0]) == 1
        for w in ("r", "l"):
            assert gold[tag + "_vel_%s_head" % w].shape == (T.C2_ROWS, 30) and gold[tag + "_vel_%s_sha" % w].shape == (32,)
    for k in ("vel_r_sha", "vel_l_sha", "err", "guard", "glist_r", "glist_l"):
        assert np.array_equal(got["c2_t16_run_" + k], got["c2_t16_cnt_" + k]), k
