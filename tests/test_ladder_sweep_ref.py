"""The swap sweep of tempered chains without a GPU (include/bh_engine_chain_ladder_sweep.h): the restatement tests/ladder_sweep_ref.py
against the rule the package already has (parallel.ladder_swap_betas), the invariants of an adapting sweep, what the adaptation does
to a badly spaced ladder on an idealised sampler, and the checks DeviceChains(ladder_adapt=) makes before it touches the engine."""
import ctypes
import os
import re

import numpy as np
import pytest

import ladder_sweep_ref as S
from conftest import REPO
from bayhunter_amd import engine as E
from bayhunter_amd import parallel as P
from bayhunter_amd.device_chains import LADDER_ADAPT_DEFAULTS, DeviceChains, ladder_adapt_options

SIZES = (1, 2, 3, 5, 64)


def interleaved_ladders(rs, sizes=SIZES):
    """ladder ids 0..K-1 of the given sizes, the members of every ladder scattered among the chains"""
    lad = np.repeat(np.arange(len(sizes)), sizes)
    return lad[rs.permutation(lad.size)]


def random_state(rs, ladder, ties=True):
    """betas in (0, 1] with a 1.0 per ladder and likes, some of both tied inside a ladder"""
    C = ladder.size
    beta = rs.uniform(0.01, 1.0, size=C)
    like = -rs.gamma(5.0, size=C) * 10.0
    for k in np.unique(ladder):
        m = np.flatnonzero(ladder == k)
        beta[m[0]] = 1.0
        if ties and m.size >= 3:
            beta[m[2]] = beta[m[1]]
            like[m[-1]] = like[m[-2]]
    return like, beta


def log_uniforms(seed, ladder, sweep):
    """the log-uniforms of a sweep in the sorted layout, as DeviceExchange and KernelExchange draw them"""
    ex = P.DeviceExchange.__new__(P.DeviceExchange)
    ex.seed, ex.N = int(seed), ladder.size
    ex.lids, ex.counts = np.unique(ladder, return_counts=True)
    return ex._log_uniforms(sweep)


def test_header_and_bindings():
    txt = open(os.path.join(REPO, "include", "bh_engine_chain_ladder_sweep.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decl = sorted(set(re.findall(r"\b(bh_[a-z_]+)\s*\(", txt)))
    assert decl == sorted(E.LADDER_SWEEP_SYMBOLS) and len(decl) == 4
    lib = ctypes.CDLL(E.LIB_PATH)
    assert all(hasattr(lib, n) for n in decl)
    lib.bh_abi_version.restype = ctypes.c_int
    assert lib.bh_abi_version() == 10                                # extension headers are outside the contract
    for hdr in sorted(os.listdir(os.path.join(REPO, "include"))):    # declared in the new header only
        if hdr != "bh_engine_chain_ladder_sweep.h":
            other = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", hdr)).read(), flags=re.S)
            assert "bh_ladder_sweep" not in other, hdr
    assert b"ladder_sweep_kernel" in open(E.LIB_PATH, "rb").read()


def test_restatement_equals_ladder_swap_betas():
    """adaptation off: 200 sweeps of alternating parity on ladders of 1, 2, 3, 5 and 64 chains, members interleaved, some betas and
    likes tied -- the betas after every sweep and the accepted count are those of parallel.ladder_swap_betas, bit for bit"""
    rs = np.random.RandomState(11)
    ladder = interleaved_ladders(rs)
    ref = S.SweepRef(ladder)
    like, beta = random_state(rs, ladder)
    nacc = 0
    for sweep in range(200):
        like = np.where(rs.uniform(size=like.size) < 0.7, -rs.gamma(5.0, size=like.size) * 10.0, like)   # (some likes stay: ties stay)
        want, n = P.ladder_swap_betas(like, beta, ladder, sweep, seed=3)
        got = ref.sweep(like, beta, log_uniforms(3, ladder, sweep), sweep % 2, int(sweep >= 100))
        assert got.tobytes() == want.tobytes(), sweep
        nacc += n
        assert int(ref.accepted.sum()) == nacc, sweep
        beta = got
    assert nacc > 100
    for k, R in enumerate(SIZES):           # every pair was proposed 50 times in each phase
        lo = int(ref.start[k])
        assert np.all(ref.proposed[:, lo:lo + R - 1] == 50) and np.all(ref.proposed[:, lo + R - 1] == 0)
    assert np.all(ref.adaptations == 0) and np.all(ref.skipped == 0)
    assert np.all(ref.accepted <= ref.proposed)


def test_invariants_of_adapting_sweeps():
    """after every adapting sweep: the ladder's ends are bitwise unchanged, the rung values strictly decrease, and the chains hold
    exactly those values; ladders of 1 and 2 chains are never adapted and never counted"""
    rs = np.random.RandomState(12)
    ladder = interleaved_ladders(rs)
    ref = S.SweepRef(ladder)
    like, beta = random_state(rs, ladder, ties=False)
    ends = [(beta[m].max(), beta[m].min()) for m in ref.members]
    n = 0
    for sweep in range(240):
        like = -rs.gamma(5.0, size=like.size) / beta
        adapt = (sweep + 1) % 4 == 0
        beta = ref.sweep(like, beta, np.log(rs.uniform(size=like.size)), sweep % 2, 0, int(adapt), S.kappa_of(n) if adapt else 0.0)
        n += int(adapt)
        for k, m in enumerate(ref.members):
            nb = ref.rung_beta[int(ref.start[k]):int(ref.start[k + 1])]
            assert nb[0].tobytes() == np.float64(ends[k][0]).tobytes() and nb[-1].tobytes() == np.float64(ends[k][1]).tobytes()
            assert np.all(np.diff(nb) < 0)
            assert np.sort(beta[m])[::-1].tobytes() == nb.tobytes()
    assert n == 60
    for k, R in enumerate(SIZES):
        assert ref.adaptations[k] + ref.skipped[k] == (60 if R >= 3 else 0)
    assert ref.adaptations[2:].min() > 0
    assert np.all(ref.wprop[np.repeat(np.asarray(SIZES) >= 3, SIZES)] == 0)      # the windows were reset by the last sweep


def test_an_adaptation_after_one_sweep_is_skipped():
    """one parity has proposed nothing: the adaptation is skipped, the betas are those of the swaps alone, the window restarts"""
    rs = np.random.RandomState(13)
    ladder = np.zeros(5, dtype=np.int64)
    like, beta = random_state(rs, ladder, ties=False)
    plain, ref = S.SweepRef(ladder), S.SweepRef(ladder)
    logu = np.log(rs.uniform(size=5))
    want = plain.sweep(like, beta, logu, 0, 0)
    got = ref.sweep(like, beta, logu, 0, 0, 1, 0.5)
    assert got.tobytes() == want.tobytes() and ref.skipped[0] == 1 and ref.adaptations[0] == 0
    assert np.all(ref.wprop == 0) and np.array_equal(ref.proposed, plain.proposed)


# ---- the rule does what it is for ---------------------------------------------------------------------------------------------------
LINEAR = np.linspace(1.0, 1e-3, 8)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_adaptation_equalises_the_rates_of_a_linear_ladder(seed):
    """The idealised sampler like = -Gamma(d/2) / beta, d = 10, 8 rungs linear in beta: 1000 windows at the defaults, then 20 000
    frozen sweeps.  Observed with this restatement, numpy.random.RandomState(seed), seeds 0..3:
        unadapted: smallest rate 0.0000 (pair 0), largest 0.809 .. 0.815
        adapted  : rates within [0.1163, 0.1585]; max - min 0.0185, 0.0273, 0.0380, 0.0314; mean 0.132 .. 0.137; no window skipped
    Thresholds: an unadapted pair below 0.01 (observed 0.0000); the adapted smallest rate above half the mean (observed >= 0.85 of
    it); max - min below 0.076 = twice the largest spread of the four seeds (0.0380)."""
    assert LADDER_ADAPT_DEFAULTS == dict(every=20, rate=0.5, lag=50.0)
    _, raw, _ = S.toy_run(LINEAR, 10, seed, 0, 20, 20000)
    assert raw.min() < 0.01
    b, rate, ref = S.toy_run(LINEAR, 10, seed, 1000, 20, 20000, rate=LADDER_ADAPT_DEFAULTS["rate"], lag=LADDER_ADAPT_DEFAULTS["lag"])
    assert ref.adaptations[0] == 1000 and ref.skipped[0] == 0
    assert b[0] == 1.0 and b[-1] == LINEAR[-1] and np.all(np.diff(b) < 0)
    assert rate.min() > 0.5 * rate.mean()
    assert rate.max() - rate.min() < 0.076


# ---- the constructor's checks: before the engine is touched -------------------------------------------------------------------------
B4 = np.array([1.0, 0.5, 0.25, 0.125])


@pytest.mark.parametrize("bad, what", [(dict(every=3), "every"), (dict(every=-2), "every"), (dict(every=2.0), "every"),
                                        (dict(every=True), "every"), (dict(rate=0.0), "rate"), (dict(rate=1.0), "rate"),
                                        (dict(rate=-0.1), "rate"), (dict(lag=0.0), "lag"), (dict(lag=-1.0), "lag"),
                                        (dict(evry=4), "unknown key"), ("on", "dict")])
def test_ladder_adapt_options_are_checked_first(bad, what):
    with pytest.raises(ValueError, match=what):
        DeviceChains(None, 4, betas=B4, swap_every=5, ladder_adapt=bad)


def test_ladder_adapt_needs_a_tempered_run_with_distinct_betas(monkeypatch):
    with pytest.raises(ValueError, match="tempered"):
        DeviceChains(None, 4, ladder_adapt={})
    with pytest.raises(ValueError, match="tempered"):
        DeviceChains(None, 4, betas=B4, swap_every=0, ladder_adapt={})
    tied = np.array([1.0, 0.5, 0.5, 0.1])
    with pytest.raises(ValueError, match="not distinct"):
        DeviceChains(None, 4, betas=tied, swap_every=5, ladder_adapt={})
    with pytest.raises(ValueError, match="not distinct"):
        DeviceChains(None, 4, betas=np.tile(tied, 2)[:8], ladder=np.repeat([7, 9], 4), swap_every=5, ladder_adapt={"every": 2})
    # distinct inside every ladder, equal across ladders: fine; every = 0 never adapts, ties are fine
    assert ladder_adapt_options({}, np.tile(B4, 2), np.repeat([0, 1], 4), 5) == LADDER_ADAPT_DEFAULTS
    assert ladder_adapt_options({"every": 0, "lag": 7}, tied, None, 5) == dict(every=0, rate=0.5, lag=7.0)
    assert ladder_adapt_options(None, None, None, 0) is None

    class TwoRanks(object):
        @staticmethod
        def is_initialized():
            return True

        @staticmethod
        def get_world_size():
            return 2

    with pytest.raises(E.EngineError, match="ranks"):
        ladder_adapt_options({}, B4, None, 5, TwoRanks)
    monkeypatch.setenv("BH_PT_HOST_EXCHANGE", "1")
    with pytest.raises(E.EngineError, match="BH_PT_HOST_EXCHANGE"):
        DeviceChains(None, 4, betas=B4, swap_every=5, ladder_adapt={})
