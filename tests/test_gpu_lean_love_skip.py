"""The trial-per-lane kernel starts a Love target's first period next to the model's slowest S velocity instead of at the scan's
start value (csrc/swd_lean.hip; the rule and its certificate: tests/test_love_scan_certificate.py).  That is scheduling only: with
the switch swd_lean_no_skip set (every round of the scan runs, as before) and unset, velocities, failure flags, guard counts and
the guard's reasons are the same bytes -- Love alone and beside Rayleigh, every trial count, the builds without and with the
counters, the site-period build, the build with the priority schedule (the bench's shape), and the models on which the rule
must not skip.  (A guarded model's row carries the reference's
bits, which differ from the short refinement's in nearly every value: equal rows pin the guard lists' members, which have no
accessor of their own.)  On the counting build, one model per launch, the Love rounds drop by exactly the restatement's m and the
Rayleigh rounds do not move."""
import numpy as np
import pytest

from bayhunter_amd import engine as E
from bayhunter_amd.synth import synth_models, prior_models, SWD_PERIODS
from test_love_scan_certificate import DC, M0_CASES, rule_of, with_vmin_at

pytestmark = pytest.mark.gpu
TRIALS = (4, 8, 16, 32, 64)
PER = SWD_PERIODS


def spec(periods=PER, waves=(2, 1)):
    yobs = 3.4 + 0.01 * periods
    return [dict(kind=E.TARGET_SWD, law=E.LAW_NOCORR, n=periods.size, x=periods, yobs=yobs, iwave=iw, igr=0) for iw in waves]


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    assert e.swd_search() == "fast" and e.swd_arith() == "fast" and e.tuning("swd_lean_no_skip") == 0
    yield e
    e.set_tuning("swd_lean_no_skip", 0)
    e.close()


def stack(*batches):
    """batches of different depths as one batch (layer-major arrays padded to the deepest)"""
    L = max(b[1].shape[0] for b in batches)
    pad = lambda a: np.vstack((a, np.zeros((L - a.shape[0], a.shape[1]))))
    return (np.concatenate([b[0] for b in batches]),) + tuple(np.hstack([pad(b[k]) for b in batches]) for k in range(1, 5))


def families(Lcap):
    """B = 252: bench-like, ragged models from a sampler's prior (2 .. 21 layers), LVZ-rich 2 .. 12 layers, the slowest layer on top /
    in the middle / in the half-space, a one-layer model (no Love root: the period fails), and the three models without a skip.
    Lcap: arrays no deeper than the launch can take on the trial-per-lane kernel (its LDS request, lean_wave_lds: at 4 trials and
    30 periods 18 layers, 14 with a row of periods per model; the test keeps to 17 and 13) -- the prior's models are drawn up to
    min(21, Lcap) layers."""
    rs = np.random.RandomState(20261101)
    one = (np.array([1], dtype=np.int32), np.zeros((1, 1)), np.full((1, 1), 6.0), np.full((1, 1), 3.5), np.full((1, 1), 2.7))
    base = prior_models(rs, 90, 12, nmin=3)
    parts = [synth_models(rs, 56, 10, lvz_frac=0.1), prior_models(rs, 56, min(21, Lcap)), synth_models(rs, 46, 12, lvz_frac=0.25, ragged=True)]
    parts += [tuple(np.ascontiguousarray(a[..., 30 * i:30 * i + 30]) for a in with_vmin_at(base, w)) for i, w in enumerate(("top", "middle", "halfspace"))]
    parts += [one] + [M0_CASES[k] for k in sorted(M0_CASES)]
    return stack(*parts)


_batches = {}


def batch_for(J, per_model_periods=False):
    Lcap = 21 if J > 4 else (13 if per_model_periods else 17)
    if Lcap not in _batches:
        _batches[Lcap] = families(Lcap)
        assert 64 <= _batches[Lcap][0].size <= 256
    return _batches[Lcap]


def with_and_without(e, call, counting=False):
    """call() with the skip (the default) and with every round of the scan: outputs, guard counts, and -- counting build -- the
    guard's reasons (words 14, 15 of the counters)"""
    out = []
    try:
        for no_skip in (0, 1):
            e.set_tuning("swd_lean_no_skip", no_skip)
            if counting:
                e.last_neval()   # (the next call's counters start from zero)
            res = call()
            assert e.last_swd_kernel() == "lean"
            c = e.debug_counters() if counting else [0] * 16
            out.append(dict(res=res, guard=e.guard_stats()[0], reasons=(c[14], c[15]), rounds=(c[1], c[4]), evals=(c[8], c[9])))
    finally:
        e.set_tuning("swd_lean_no_skip", 0)
    return out


def assert_same(a, b, what):
    for k, (x, y) in enumerate(zip(a["res"], b["res"])):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)
    assert a["guard"] == b["guard"] and a["reasons"] == b["reasons"], what


@pytest.mark.parametrize("counting", [False, True])
@pytest.mark.parametrize("J", TRIALS)
def test_love_alone_and_beside_rayleigh_same_bytes(eng, J, counting):
    nlay, h, vp, vs, rho = batch_for(J)
    B = nlay.size
    noise = np.tile([0.0, 0.05, 0.0, 0.05], (B, 1))
    eng.set_swd_trials(J)
    eng.set_instrumentation(False, counting)
    try:
        alone = with_and_without(eng, lambda: eng.swd_batch(nlay, h, vp, vs, rho, PER, 1, 0), counting)
        assert_same(alone[0], alone[1], "Love alone")
        v, err = alone[0]["res"]
        assert err[-4] != 0 and not v[-4].any()                       # the one-layer model: the first period fails, a zero row
        assert (err == 0).sum() > 0.5 * B and sum(alone[0]["guard"]) > 0    # (the batch holds searches that end and guarded ones)
        eng.set_targets(spec())
        both = with_and_without(eng, lambda: eng.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True), counting)
        assert_same(both[0], both[1], "Rayleigh + Love")
        if counting:   # the skip is Love's alone, and it does skip: evaluations consumed, Rayleigh / Love (the re-run launch of the
            #            guarded models writes its own clocks into the words of the rounds: those are read at B = 1, below)
            assert both[0]["evals"][1] < both[1]["evals"][1] and alone[0]["evals"][1] < alone[1]["evals"][1]
            assert both[0]["evals"][0] == both[1]["evals"][0] > 0 and alone[0]["evals"][0] == alone[1]["evals"][0] == 0
    finally:
        eng.set_instrumentation(False, False)
        eng.set_swd_trials(0)


@pytest.mark.parametrize("J", TRIALS)
def test_a_single_period(eng, J):
    nlay, h, vp, vs, rho = batch_for(J)
    eng.set_swd_trials(J)
    try:
        for period in (2.0, 37.0):
            r = with_and_without(eng, lambda: eng.swd_batch(nlay, h, vp, vs, rho, np.array([period]), 1, 0))
            assert_same(r[0], r[1], period)
    finally:
        eng.set_swd_trials(0)


@pytest.mark.parametrize("counting", [False, True])
@pytest.mark.parametrize("J", TRIALS)
def test_two_sites_with_different_first_periods_through_the_site_period_build(eng, J, counting):
    nlay, h, vp, vs, rho = batch_for(J, per_model_periods=True)
    B = nlay.size
    sets = (np.linspace(2.0, 60.0, 30), np.linspace(7.0, 45.0, 12))
    cap = 30
    n = np.array([[p.size, p.size] for p in sets], dtype=np.int32)
    x, yobs = np.zeros((2, 2 * cap)), np.zeros((2, 2 * cap))
    for s, p in enumerate(sets):
        for t in range(2):
            x[s, t * cap:t * cap + p.size] = p
            yobs[s, t * cap:t * cap + p.size] = 3.4 + 0.01 * p
    site = (np.arange(B) % 2).astype(np.int32)
    noise = np.tile([0.0, 0.05, 0.0, 0.05], (B, 1))
    eng.set_swd_trials(J)
    eng.set_instrumentation(False, counting)
    try:
        eng.set_targets(spec(np.ones(cap)))
        eng.set_sites_x(n, x, yobs)
        r = with_and_without(eng, lambda: eng.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True), counting)
        assert_same(r[0], r[1], "site periods")
        assert any(l["family"] == "lean" and l["role"] == "main" for l in eng.last_swd_launches())
        if counting:
            assert r[0]["evals"][1] < r[1]["evals"][1] and r[0]["evals"][0] == r[1]["evals"][0] > 0
        ymod = r[0]["res"][3]
        assert not ymod[site == 1][:, 12:cap].any() and ymod[site == 0][:, :cap].any()
    finally:
        eng.set_instrumentation(False, False)
        eng.set_swd_trials(0)
        eng.set_targets(spec())


@pytest.mark.parametrize("counting", [False, True])
def test_the_bench_shape_with_the_priority_schedule(eng, counting):
    """B = 4096, both targets, 16 trials: on 256 CUs the launch of one Rayleigh and one Love wavefront per SIMD, which has a build of
    its own (the priority schedule: SwdMultiArgs::lean_prio) -- beyond the sizes above, because no smaller batch reaches that build"""
    nlay, h, vp, vs, rho = synth_models(np.random.RandomState(4242), 4096, 10, lvz_frac=0.1)
    noise = np.tile([0.0, 0.05, 0.0, 0.05], (4096, 1))
    eng.set_swd_trials(16)
    eng.set_instrumentation(False, counting)
    try:
        eng.set_targets(spec())
        r = with_and_without(eng, lambda: eng.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True), counting)
        assert_same(r[0], r[1], "bench shape")
        main = [l for l in eng.last_swd_launches() if l["role"] == "main"]
        assert len(main) == 1 and main[0]["family"] == "lean"
        print("priority time slice of the launch (0: as dispatched): %d" % main[0]["fair"])
        if counting:
            assert r[0]["evals"][1] < r[1]["evals"][1] and r[0]["evals"][0] == r[1]["evals"][0] > 0
    finally:
        eng.set_instrumentation(False, False)
        eng.set_swd_trials(0)


def clear_models(oracle, J, want=3):
    """bench-like models whose m stands a tenth of a step away from both of its neighbours, with the restatement's m"""
    models = synth_models(np.random.RandomState(4100 + J), 64, 10, lvz_frac=0.1)
    omega = 2.0 * np.pi / PER[0]
    out = []
    for i in range(64):
        cm, m, bm, bound, ok_q, ok_v = rule_of(oracle, models, i, omega, J)
        lim = float(np.float32(models[3][:, i]).astype(float).min()) - DC
        if m > 0 and bm + 2.0 * DC <= lim - 0.1 * DC and (bm + J * DC) + 2.0 * DC > lim + 0.1 * DC:
            out.append((tuple(np.ascontiguousarray(a[..., i:i + 1]) for a in models), m))
    assert len(out) >= want
    return out[:want]


@pytest.mark.parametrize("J", TRIALS)
def test_the_love_rounds_drop_by_the_restatements_count(eng, oracle, J):
    """B = 1 on the counting build: one Love (and one Rayleigh) wavefront, whose rounds the counters hold"""
    eng.set_swd_trials(J)
    eng.set_instrumentation(False, True)
    try:
        for (nlay, h, vp, vs, rho), m in clear_models(oracle, J):
            eng.set_targets(spec())
            noise = np.array([[0.0, 0.05, 0.0, 0.05]])
            both = with_and_without(eng, lambda: eng.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True), True)
            alone = with_and_without(eng, lambda: eng.swd_batch(nlay, h, vp, vs, rho, PER, 1, 0), True)
            for r in (both, alone):
                assert_same(r[0], r[1], J)
                assert r[0]["guard"] == [0] * len(r[0]["guard"]) and not r[0]["res"][-1 if r is alone else 2].any()   # ends, unguarded
                print("J %d: Love rounds %d -> %d (m = %d), Rayleigh rounds %d -> %d" % (J, r[1]["rounds"][1], r[0]["rounds"][1], m, r[1]["rounds"][0], r[0]["rounds"][0]))
                assert r[1]["rounds"][1] - r[0]["rounds"][1] == m
                assert r[1]["rounds"][0] == r[0]["rounds"][0]
            assert both[0]["rounds"][0] > 0 and alone[0]["rounds"][0] == 0
    finally:
        eng.set_instrumentation(False, False)
        eng.set_swd_trials(0)
