"""The fast arithmetic of the dispersion kernels keeps its BITS (csrc/swd_fa.h, csrc/swd_lean.hip): the functions of namespace fa,
the secular evaluators and whole searches against tests/golden/lean_eval_bits.npz, which tools/record_lean_eval_bits.py recorded
-- inputs and outputs together -- with the library of the commit before the layer steps lost their copies of the polynomials'
constants (fa::fma_leaf).  Outputs are compared as uint64 views; where the golden holds NaN the value must
be NaN (the payload is free).  The calls are the recorder's own (compute(), imported from the tool); nothing is drawn here."""
import os
import sys

import numpy as np
import pytest

from conftest import REPO, golden

sys.path.insert(0, os.path.join(REPO, "tools"))
import record_lean_eval_bits as T  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return {k: v for k, v in golden("lean_eval_bits.npz").items()}


@pytest.fixture(scope="module")
def got(engine, gold):
    """every recorded call once, shared by the tests below (the search and arithmetic it selects are the engine's defaults; the
    suite's autouse fixture puts back what it had set)"""
    search, arith = engine.swd_search(), engine.swd_arith()
    out = T.compute(engine, gold)
    engine.set_swd_search(search)
    engine.set_swd_arith(arith)
    return out


def _bits_differ(new, old):
    """indices where the bits differ, NaN against NaN excepted"""
    assert new.shape == old.shape and new.dtype == old.dtype == np.float64
    both_nan = np.isnan(new) & np.isnan(old)
    return np.flatnonzero((new.view(np.uint64) != old.view(np.uint64)) & ~both_nan)


@pytest.mark.parametrize("name", ["rcp", "rcp1", "sqrt", "rsqrt", "sin", "cos", "expneg"])
def test_functions(got, gold, name):
    x = gold["fn_%s_x" % {"sin": "sincos", "cos": "sincos", "expneg": "expneg"}.get(name, "pos")]
    bad = _bits_differ(got["fn_" + name], gold["fn_" + name])
    print("fa::%s: %d inputs, %d differ" % (name, x.size, bad.size))
    assert bad.size == 0, (name, x[bad[:8]], got["fn_" + name][bad[:8]], gold["fn_" + name][bad[:8]])


@pytest.mark.parametrize("ifunc", [1, 2])
@pytest.mark.parametrize("ev", [1, 2])
def test_secular(got, gold, ev, ifunc):
    """2, 3, 10, 11 and 32 layers and the model with a poisoning layer; mtop = mmax (`top`: the lean evaluator's one-depth case) and
    mmax + 1 (`rag`)"""
    keys = [k for k in sorted(gold) if k.startswith("sec_") and ("_%d_ev%d_" % (ifunc, ev)) in k]
    assert len(keys) == (12 if ev == 1 else 11), keys
    nnan = 0
    for k in keys:
        bad = _bits_differ(got[k], gold[k])
        nnan += int(np.isnan(gold[k]).sum())
        assert bad.size == 0, (k, bad[:8], got[k][bad[:8]], gold[k][bad[:8]])
    print("evaluator %d, %s: %d sets of 64 points, %d NaN among them, all bits equal" % (ev, {1: "Love", 2: "Rayleigh"}[ifunc], len(keys), nnan))


@pytest.mark.parametrize("trials", T.TRIALS)
@pytest.mark.parametrize("pop", ["synth", "prior"])
def test_searches(got, gold, pop, trials):
    """swd_batch, default search and arithmetic, trials pinned: velocities, failure flags and the guard's counts"""
    for wave in ("r", "l"):
        key = "run_%s_%s_t%d" % (pop, wave, trials)
        v, g = got[key + "_vel"], gold[key + "_vel"]
        assert v.dtype == g.dtype == np.float32
        # (binary32 holds the velocities exactly -- compute() asserts it -- so these are the bits of the binary64 the kernel wrote)
        bad = np.argwhere(v.view(np.uint32) != g.view(np.uint32))
        assert bad.shape[0] == 0, (key, bad[:8])
        assert np.array_equal(got[key + "_err"], gold[key + "_err"]), key
        assert np.array_equal(got[key + "_guard"], gold[key + "_guard"]), (key, got[key + "_guard"], gold[key + "_guard"])
        print("%s: %d models, %d failed, guard %s" % (key, v.shape[0], int((gold[key + "_err"] != 0).sum()), gold[key + "_guard"].tolist()))
