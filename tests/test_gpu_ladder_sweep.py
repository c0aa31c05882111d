"""The swap sweep of tempered chains on the GPU (include/bh_engine_chain_ladder_sweep.h): the kernel, driven through engine.LadderSweep
with synthetic tensors, against the restatement tests/ladder_sweep_ref.py -- the betas after every sweep and every counter, bit for
bit --, its refusals, and DeviceChains(ladder_adapt=) end to end: counting only, the run is the run without ladder_adapt; adapting,
the recorded betas keep their ends, stay ordered and are frozen before the first posterior sample."""
import numpy as np
import pytest

import ladder_sweep_ref as S
from conftest import golden
from test_ladder_sweep_ref import SIZES, interleaved_ladders, log_uniforms, random_state
from bayhunter_amd import engine as E
from bayhunter_amd import parallel as P
from bayhunter_amd.device_chains import DeviceChains

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    return E.Engine(0)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")


def same_counters(plan, ref):
    got = plan.read()
    for k in ("proposed", "accepted", "adaptations", "skipped"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], getattr(ref, k)), k
    assert got["rung_beta"].tobytes() == ref.rung_beta.tobytes()
    return got


class Pair(object):
    """the kernel's plan and the restatement's, fed the same sweeps; the betas are compared after every sweep"""

    def __init__(self, engine, ladder, beta):
        self.plan, self.ref = E.LadderSweep(engine, ladder), S.SweepRef(ladder)
        self.beta = np.array(beta, dtype=np.float64)
        self.dbeta = dev(self.beta)

    def sweep(self, like, logu, parity, phase, adapt=0, kappa=0.0):
        want = self.ref.sweep(like, self.beta, logu, parity, phase, adapt, kappa)
        self.plan.run(dev(like), self.dbeta, dev(logu), parity, phase, adapt, kappa)
        got = self.dbeta.cpu().numpy()
        assert got.tobytes() == want.tobytes(), (parity, phase, adapt)
        self.beta = want
        return want


def test_counting_sweeps_equal_the_restatement_and_ladder_swap_betas(engine):
    """adapt = 0: the ladders of the CPU test (1, 2, 3, 5 and 64 chains, interleaved, tied betas and likes), likes with NaN and
    +-inf, 200 sweeps of alternating parity, the second hundred counted as main phase"""
    rs = np.random.RandomState(11)
    ladder = interleaved_ladders(rs)
    like, beta = random_state(rs, ladder)
    pair = Pair(engine, ladder, beta)
    odd = np.array([np.nan, np.inf, -np.inf])
    for sweep in range(200):
        like = np.where(rs.uniform(size=like.size) < 0.7, -rs.gamma(5.0, size=like.size) * 10.0, like)
        like = np.where(rs.uniform(size=like.size) < 0.1, odd[rs.randint(3, size=like.size)], like)
        before = pair.beta
        got = pair.sweep(like, log_uniforms(3, ladder, sweep), sweep % 2, int(sweep >= 100))
        with np.errstate(invalid="ignore"):           # (inf - inf and 0 * inf in the NumPy form: NaN, which compares false)
            assert got.tobytes() == P.ladder_swap_betas(like, before, ladder, sweep, seed=3)[0].tobytes(), sweep
    got = same_counters(pair.plan, pair.ref)
    assert got["accepted"].sum() > 100 and np.all(got["adaptations"] == 0) and np.all(got["skipped"] == 0)
    for k, R in enumerate(SIZES):
        lo = int(pair.plan.start[k])
        assert np.all(got["proposed"][:, lo:lo + R - 1] == 50) and np.all(got["proposed"][:, lo + R - 1] == 0)


ADAPT_SIZES = (3, 2, 1, 64, 4)


@pytest.mark.parametrize("every", [2, 4, 20])
def test_adapting_sweeps_equal_the_restatement(engine, every):
    """ladders of 3 (the smallest that adapts), 2 and 1 (untouched, never counted), 64, and one of 4 with a gap of 1e-9 of its span --
    below the floor 0x1p-20 * span, which then binds -- in one plan; an adaptation every 2, 4 and 20 sweeps with the host's gain"""
    rs = np.random.RandomState(20 + every)
    ladder = interleaved_ladders(rs, ADAPT_SIZES)
    like, beta = random_state(rs, ladder, ties=False)
    four = np.flatnonzero(ladder == 4)
    beta[four] = [0.1, 0.5 - 1e-9, 1.0, 0.5]
    pair = Pair(engine, ladder, beta)
    n, floor_bound = 0, False
    for sweep in range(120):
        like = -rs.gamma(5.0, size=beta.size) / pair.beta
        adapt = (sweep + 1) % every == 0
        lo = int(pair.ref.start[4])
        gap = pair.ref.rung_beta[lo + 1] - pair.ref.rung_beta[lo + 2] if sweep else 1e-9
        pair.sweep(like, np.log(rs.uniform(size=beta.size)), sweep % 2, 0, int(adapt), S.kappa_of(n) if adapt else 0.0)
        n += int(adapt)
        if adapt and not floor_bound and pair.ref.adaptations[4] == 1 and gap < 2e-9:
            after = pair.ref.rung_beta[lo + 1] - pair.ref.rung_beta[lo + 2]
            assert after > 100 * gap                   # 1e-9 of the span became the floor's share of it
            floor_bound = True
    assert floor_bound
    got = same_counters(pair.plan, pair.ref)
    for k, R in enumerate(ADAPT_SIZES):
        assert got["adaptations"][k] + got["skipped"][k] == (120 // every if R >= 3 else 0)
    assert np.all(got["adaptations"][[0, 3, 4]] > 0)
    for k in (1, 2):                                   # the ladders of 2 and 1 hold what they started with
        m = pair.plan.members[k]
        assert np.sort(pair.beta[m]).tobytes() == np.sort(beta[m]).tobytes()
    # two more sweeps counted as main phase: the temperatures are frozen
    rung = got["rung_beta"].copy()
    for sweep in (120, 121):
        pair.sweep(-rs.gamma(5.0, size=beta.size) / pair.beta, np.log(rs.uniform(size=beta.size)), sweep % 2, 1)
    assert same_counters(pair.plan, pair.ref)["rung_beta"].tobytes() == rung.tobytes()


def test_an_adaptation_after_a_single_sweep_is_skipped(engine):
    """the other parity's pairs have proposed nothing: skipped, the betas are those of the swaps alone; then a full window adapts"""
    rs = np.random.RandomState(31)
    ladder = np.array([0, 1, 0, 1, 0, 1, 0, 0])
    like, beta = random_state(rs, ladder, ties=False)
    pair, plain = Pair(engine, ladder, beta), S.SweepRef(ladder)
    logu = np.log(rs.uniform(size=8))
    got = pair.sweep(like, logu, 0, 0, 1, 0.5)
    assert got.tobytes() == plain.sweep(like, beta, logu, 0, 0).tobytes()
    r = same_counters(pair.plan, pair.ref)
    assert list(r["skipped"]) == [1, 1] and list(r["adaptations"]) == [0, 0]
    pair.sweep(like, logu, 1, 0)
    pair.sweep(like, logu, 0, 0, 1, 0.5)
    r = same_counters(pair.plan, pair.ref)
    assert list(r["skipped"]) == [1, 1] and list(r["adaptations"]) == [1, 1]


def test_new_values_out_of_order_leave_the_ladder(engine):
    """The guard of step 3: the recurrence nb[r] = nb[r-1] - g2[r-1] rounds at the magnitude of the betas, the gaps are held above
    2^-20 of the SPAN -- a ladder whose span is far below its betas' magnitude can lose a gap to that rounding.  Here
    b = [1.5, 1.5 - 2^-52, 1.5 - 2^-40] (the floor, 2^-60, is far below an ulp), pair 0 rejected and pair 1 accepted in the window,
    kappa = 0.99: the first gap (one ulp) shrinks to a third of an ulp, nb[1] rounds to nb[0], and the sweep is counted as skipped
    with the betas unchanged.  With a span of 2^-30 the floor is 4 ulps and the same window adapts.  (Ladders
    of a run start at beta = 1 with spans of order 1: there the floor keeps every gap at 2^-20, 2^32 ulps.)"""
    b = np.array([1.5, 1.5 - 2.0 ** -52, 1.5 - 2.0 ** -40])
    assert b[0] > b[1] > b[2]
    ladder = np.zeros(3, dtype=np.int64)
    pair = Pair(engine, ladder, b[[1, 2, 0]])
    like = np.zeros(3)
    no, yes = np.full(3, np.inf), np.full(3, -np.inf)
    pair.sweep(like, no, 0, 0)                         # pair (0, 1): proposed, rejected
    before = pair.sweep(like, yes, 1, 0)               # pair (1, 2): proposed, accepted
    after = pair.sweep(like, no, 0, 0, 1, 0.99)
    assert pair.ref.skipped[0] == 1 and pair.ref.adaptations[0] == 0 and np.all(pair.ref.wprop == 0)   # the branch was reached
    assert after.tobytes() == before.tobytes()
    same_counters(pair.plan, pair.ref)
    assert S.adapted(list(b), [0, 1], [2, 1], 0.99) is None and S.adapted(list(b), [0, 1], [2, 1], 0.5) is not None
    assert S.adapted([1.5, b[1], 1.5 - 2.0 ** -30], [0, 1], [2, 1], 0.99) is not None


def test_refusals_write_nothing(engine):
    with pytest.raises(E.EngineError, match=r"\(-1\).*every id used"):
        E.LadderSweep(engine, [0, 0, 2, 2])            # id 1 is unused
    with pytest.raises(E.EngineError, match=r"\(-1\).*0\.\.K-1"):
        E.LadderSweep(engine, [0, 1, 2, 1], K=2)       # an id beyond K
    with pytest.raises(E.EngineError, match=r"\(-1\)"):
        E.LadderSweep(engine, [0, -1, 0])
    with pytest.raises(E.EngineError, match=r"\(-4\).*BH_LADDER_MAXRUNGS"):
        E.LadderSweep(engine, [0] * 65 + [1])
    E.LadderSweep(engine, [0] * 64 + [1]).close()      # 64 is the limit
    rs = np.random.RandomState(5)
    ladder = np.zeros(4, dtype=np.int64)
    like, beta = random_state(rs, ladder, ties=False)
    plan = E.LadderSweep(engine, ladder)
    dbeta, dlike, dlogu = dev(beta), dev(like), dev(np.full(4, -np.inf))
    with pytest.raises(E.EngineError, match=r"\(-1\).*frozen"):
        plan.run(dlike, dbeta, dlogu, 0, 1, 1, 0.5)    # adapt with phase 1
    for parity, phase in ((2, 0), (0, 2), (-1, 0)):
        with pytest.raises(E.EngineError, match=r"\(-1\)"):
            plan.run(dlike, dbeta, dlogu, parity, phase)
    with pytest.raises(ValueError, match="logu"):
        plan.run(dlike, dbeta, dev(np.zeros(3)), 0, 0)
    assert dbeta.cpu().numpy().tobytes() == beta.tobytes()
    got = plan.read()
    assert all(not np.any(got[k]) for k in ("proposed", "accepted", "adaptations", "skipped", "rung_beta"))


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def tempered(tmp, **kw):
    """the tempered set-up of tests/test_gpu_chain_diag_ladders.py: two ladders of four temperatures on the golden chain targets"""
    from test_gpu_chains import SETUPS, make_targets
    g = golden("chain_golden.npz")
    su = SETUPS["exp"]
    init = dict(su["init"], iter_burnin=kw.pop("iter_burnin"), iter_main=kw.pop("iter_main"), maxmodels=kw.pop("maxmodels"),
                savepath=str(tmp))
    ladder = np.repeat(np.arange(2), 4)
    betas = np.tile(1.0 / np.geomspace(1.0, 20.0, 4), 2)
    return DeviceChains(make_targets(g), 8, init, su["priors"], seed=5, betas=betas, ladder=ladder, **kw), betas


def same_dict(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), k


def sweeps_of(burnin, main, swap_every):
    """(sweeps of the burn-in, sweeps of the main phase): a sweep follows every iteration count iiter that swap_every divides,
    iiter in (-burnin, main]; those with iiter <= 0 are the burn-in's"""
    at = [i for i in range(-burnin + 1, main + 1) if i % swap_every == 0]
    return len([i for i in at if i <= 0]), len([i for i in at if i > 0])


def test_counting_run_is_the_run_without_ladder_adapt(tmp_path):
    kw = dict(iter_burnin=180, iter_main=240, maxmodels=60, swap_every=5)
    plain, _ = tempered(tmp_path, **kw)
    plain.run()
    with pytest.raises(E.EngineError, match="ladder_adapt"):
        plain.ladder_swaps()
    counted, betas = tempered(tmp_path, ladder_adapt={"every": 0}, **kw)
    counted.run()
    for phase in ("p1", "p2"):
        same_dict(counted.samples(phase), plain.samples(phase))
    same_dict(counted.state_host(), plain.state_host())
    assert counted.nswaps == plain.nswaps > 0
    sw = counted.ladder_swaps()
    assert list(sw["ids"]) == [0, 1] and [list(m) for m in sw["members"]] == [[0, 1, 2, 3], [4, 5, 6, 7]]
    assert sum(int(a.sum()) for a in sw["accepted"]) == counted.nswaps
    n1, n2 = sweeps_of(180, 240, 5)
    assert n1 + n2 == counted.sweep
    for k in range(2):
        assert sw["proposed"][k].dtype == np.int64 and sw["proposed"][k].shape == (2, 3)
        # sweeps s = 0 .. n1-1 are the burn-in's: pairs 0 and 2 on even s, pair 1 on odd s
        even1, even = (n1 + 1) // 2, (n1 + n2 + 1) // 2
        assert sw["proposed"][k].tolist() == [[even1, n1 - even1, even1], [even - even1, n2 - (even - even1), even - even1]]
        assert sw["betas"][k].tobytes() == sw["betas0"][k].tobytes() == np.sort(betas[:4])[::-1].tobytes()
        with np.errstate(invalid="ignore"):
            assert np.array_equal(sw["rate"][k], sw["accepted"][k] / sw["proposed"][k].astype(float), equal_nan=True)
    assert not np.any(sw["adaptations"]) and not np.any(sw["skipped"])


def test_adapting_run_freezes_ordered_ladders_before_the_main_phase(tmp_path):
    every, swap_every, burnin, main = 4, 2, 120, 80
    dc, betas = tempered(tmp_path, iter_burnin=burnin, iter_main=main, maxmodels=main, swap_every=swap_every, record="device",
                         ladder_adapt={"every": every})
    dc.run()
    assert dc.thinning == 1
    sw = dc.ladder_swaps()
    n1, n2 = sweeps_of(burnin, main, swap_every)
    assert n1 + n2 == dc.sweep
    assert np.all(sw["adaptations"] + sw["skipped"] == n1 // every) and np.all(sw["adaptations"] > 0)
    lo = np.float64(betas[:4].min())
    for k in range(2):
        cols = slice(4 * k, 4 * k + 4)
        rows = {ph: np.sort(dc.samples(ph)["beta"][:, cols], axis=1)[:, ::-1] for ph in ("p1", "p2")}
        assert rows["p1"].shape == (burnin, 4) and rows["p2"].shape == (main, 4)
        for ph in ("p1", "p2"):
            assert np.all(np.diff(rows[ph], axis=1) < 0)
            assert np.all(rows[ph][:, 0] == 1.0) and rows[ph][:, -1].tobytes() == np.full(rows[ph].shape[0], lo).tobytes()
        assert all(r.tobytes() == sw["betas"][k].tobytes() for r in rows["p2"])
        assert len({r.tobytes() for r in rows["p1"]}) <= sw["adaptations"][k] + 1
        assert sw["betas0"][k].tobytes() == np.sort(betas[:4])[::-1].tobytes() and sw["betas"][k].tobytes() != sw["betas0"][k].tobytes()
        assert sw["proposed"][k][0].sum() + sw["proposed"][k][1].sum() > 0 and np.all(sw["accepted"][k] <= sw["proposed"][k])
    assert sum(int(a.sum()) for a in sw["accepted"]) == dc.nswaps
    cold = dc.samples("p2", cold_only=True)
    assert cold["likes"].shape == (main, 2)
    diag = dc.ladder_diagnostics()
    assert np.all(diag["ladders"]["occupancy"].sum(axis=1) == main)
