"""The schedule of the trial-per-lane dispersion launch is scheduling only: which models share a wavefront, which Love group sits
beside which Rayleigh group on a SIMD (swd_lean_kernel's opposite order, which follows the dispatcher's two passes of workgroups
where the launch is exactly two workgroups per CU) and which of a SIMD's two wavefronts has the high issue priority in a time
slice (SwdMultiArgs::lean_prio) must not show in a single bit of a result.

c2's targets on an engine of its own, default search and arithmetic, the trials pinned to 16 (4 models per wavefront), so that
B = 4096 with both targets is the launch of 2048 wavefronts in which the priorities and the pass-aware pairing act (on 256 CUs),
and every smaller batch, and a target alone, is a launch in which they must stay off.

The ordering launch in front of it is pinned too: what it wrote is read back (bh_engine_last_swd_perm) and must hold every model
once, inside its XCD block where the order is blocked; the words it zeroes for the call must be zeroed; a sampler's windows
walk the same trajectory in the order as given; a batch beyond the sorted list's capacity takes the depth order."""
import numpy as np
import pytest

from bayhunter_amd import engine as E
from bayhunter_amd.synth import synth_models, prior_models, SWD_PERIODS

pytestmark = pytest.mark.gpu
L = 10
TRIALS = 16


def spec(nt):
    yobs = 3.4 + 0.01 * SWD_PERIODS
    return [dict(kind=E.TARGET_SWD, law=E.LAW_NOCORR, n=SWD_PERIODS.size, x=SWD_PERIODS, yobs=yobs, iwave=iw, igr=0) for iw in (2, 1)][:nt]


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    assert e.swd_search() == "fast" and e.swd_arith() == "fast"
    e.set_swd_trials(TRIALS)
    e.set_targets(spec(2))
    yield e
    e.close()


def evaluate(e, models, Lmax=L):
    """evaluate_batch_dev on device-resident layer-major arrays; (logL, misfits, err, ymod) back on the host"""
    import torch
    dev = torch.device("cuda", 0)
    B, nt = models[0].size, e.ntargets
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in models]
    noise = np.zeros((B, 2 * nt))
    noise[:, 1::2] = 0.02
    d_noise = torch.from_numpy(noise).to(dev)
    out = [torch.zeros(B, dtype=torch.float64, device=dev), torch.zeros((B, nt + 1), dtype=torch.float64, device=dev),
           torch.full((B,), -1, dtype=torch.int32, device=dev), torch.zeros((B, e.ldy), dtype=torch.float64, device=dev)]
    e.evaluate_batch_dev(B, Lmax, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), B, 1,
                         d_noise.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), ymod=out[3].data_ptr(),
                         stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def same_bits(a, b):
    return all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def acts(e):
    """the priority time slice the main launch of the last call ran with (0: as dispatched)"""
    main = [r for r in e.last_swd_launches() if r["role"] == "main"]
    assert len(main) == 1 and main[0]["family"] == "lean"
    return main[0]["fair"]


def two_per_cu(B, nt):
    """the launch is two workgroups of four wavefronts per CU, one Rayleigh and one Love wavefront on every SIMD"""
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    waves = nt * ((B + 3) // 4)
    return nt == 2 and waves % 4 == 0 and ncu < waves // 4 <= 2 * ncu


@pytest.fixture(scope="module")
def c2_batch():
    return synth_models(np.random.RandomState(4242), 4096, L, lvz_frac=0.1)


def test_the_priority_schedule_and_the_pairing_leave_every_bit(eng, c2_batch):
    """B = 4096, both targets: the default schedule against the launch as dispatched (no priorities, the plain opposite order),
    each switch alone, other shares and slices, the order as given and the order by depth"""
    try:
        got = evaluate(eng, c2_batch)
        assert eng.last_swd_order()[:2] == ("length", 8)
        assert (acts(eng) > 0) == two_per_cu(4096, 2)
        assert np.all(got[2] >= 0) and np.isfinite(got[0][got[2] == 0]).all() and np.count_nonzero(got[3]) > 0.99 * got[3].size
        for share, slc, no_half in ((0, 0, 1), (0, 0, 0), (7, 0, 1), (1, 12, 0), (8, 20, 0), (4, 8, 0)):
            eng.set_tuning("swd_lean_share", share)
            eng.set_tuning("swd_lean_slice", slc)
            eng.set_tuning("swd_lean_no_half", no_half)
            other = evaluate(eng, c2_batch)
            assert (acts(eng) > 0) == (share > 0 and two_per_cu(4096, 2)) and (slc == 0 or acts(eng) in (0, slc))
            assert same_bits(got, other), (share, slc, no_half)
        eng.set_tuning("swd_lean_share", 7)
        eng.set_tuning("swd_lean_slice", 0)
        eng.set_tuning("swd_lean_no_half", 0)
        eng.set_model_order(sort_by_depth=False)
        as_given = evaluate(eng, c2_batch)
        assert eng.last_swd_order() == ("none", 0, set()) and (acts(eng) > 0) == two_per_cu(4096, 2)
        assert same_bits(got, as_given)
        eng.set_model_order(sort_by_depth=True)
        eng.set_tuning("swd_lean_no_sort", 1)
        by_depth = evaluate(eng, c2_batch)
        assert eng.last_swd_order()[0] == "depth"
        assert same_bits(got, by_depth)
    finally:
        eng.set_model_order(sort_by_depth=True)
        for name, v in (("swd_lean_share", 7), ("swd_lean_slice", 0), ("swd_lean_no_half", 0), ("swd_lean_no_sort", 0)):
            eng.set_tuning(name, v)


@pytest.mark.parametrize("B", [1, 5, 32, 33, 67, 1024, 1032])
@pytest.mark.parametrize("nt", [2, 1])
def test_every_other_launch_runs_as_dispatched_and_every_order_gives_the_same_bits(eng, B, nt):
    models = synth_models(np.random.RandomState(5200 + B + nt), B, L, lvz_frac=0.1)
    try:
        if nt != 2:
            eng.set_targets(spec(nt))
        got = evaluate(eng, models)
        assert eng.last_swd_kernel() == "lean" and acts(eng) == 0
        assert np.all(got[2] >= 0) and np.isfinite(got[0][got[2] == 0]).all()
        eng.set_model_order(sort_by_depth=False)
        as_given = evaluate(eng, models)
        assert eng.last_swd_order() == ("none", 0, set()) and acts(eng) == 0
        assert same_bits(got, as_given)
        eng.set_model_order(sort_by_depth=True)
        eng.set_tuning("swd_lean_no_sort", 1)
        by_depth = evaluate(eng, models)
        assert eng.last_swd_order()[0] == ("depth" if B > 1 else "none")
        assert same_bits(got, by_depth)
    finally:
        eng.set_tuning("swd_lean_no_sort", 0)
        eng.set_model_order(sort_by_depth=True)
        if nt != 2:
            eng.set_targets(spec(2))


def test_one_target_alone_at_the_c2_batch(eng, c2_batch):
    """a target alone has no partner target on its SIMDs: as dispatched, and the velocities it gives are those of the call with both"""
    both = evaluate(eng, c2_batch)
    try:
        eng.set_targets(spec(1))
        one = evaluate(eng, c2_batch)
        assert acts(eng) == 0
        n = SWD_PERIODS.size
        assert one[3][:, :n].tobytes() == np.ascontiguousarray(both[3][:, :n]).tobytes()
    finally:
        eng.set_targets(spec(2))


def test_mixed_depths_fall_back_to_the_depth_order(eng):
    """2 .. 21 layers from a sampler's prior, 4096 models, both targets: ordered by depth (deepest first) inside the ordering launch,
    the priorities on (the launch has the shape), the bits those of the order as given"""
    Lm = 21
    models = prior_models(np.random.RandomState(77), 4096, Lm)
    assert models[0].min() == 2 and models[0].max() == Lm
    try:
        got = evaluate(eng, models, Lm)
        assert eng.last_swd_order()[0] == "length" and (acts(eng) > 0) == two_per_cu(4096, 2)
        eng.set_model_order(sort_by_depth=False)
        as_given = evaluate(eng, models, Lm)
        assert same_bits(got, as_given)
        eng.set_model_order(sort_by_depth=True)
        eng.set_tuning("swd_lean_share", 0)
        plain = evaluate(eng, models, Lm)
        assert acts(eng) == 0 and same_bits(got, plain)
    finally:
        eng.set_tuning("swd_lean_share", 7)
        eng.set_model_order(sort_by_depth=True)


# ---- the ordering launch itself: what it wrote is an order, and the call's words are zeroed ------------------------------------------
ORDER_SHAPES = [1, 5, 32, 33, 67, 1024, 1032, 4096]


def blocked(B, nt):
    """the plan's rule for an order inside eight XCD blocks (plan_swd): whole wavefronts that divide over 8 XCDs x the target's
    wavefronts per workgroup"""
    return B % 4 == 0 and B % 8 == 0 and (B // 4) % (8 * (2 if nt == 2 else 4)) == 0


def check_order(e, B, nt, nlay):
    order, wgs, _ = e.last_swd_order()
    if B == 1:
        assert order == "none" and e.last_swd_perm(0, B) is None
        return
    assert order == "length" and wgs == (8 if blocked(B, nt) else 1)
    for t in range(nt):
        perm = e.last_swd_perm(t, B)
        assert perm is not None and perm.shape == (B,)
        assert np.array_equal(np.sort(perm), np.arange(B)), t                      # every model exactly once
        if nlay.min() != nlay.max():
            assert np.all(np.diff(nlay[perm]) <= 0)                                # mixed depths: deepest first
        elif wgs == 8:                                                             # equal depths, blocked: wavefront w runs on XCD
            wid = np.arange(B) // 4                                                # (w >> 1) & 7 (two targets) / (w >> 2) & 7 and
            xcd = (wid >> 1) & 7 if nt == 2 else (wid >> 2) & 7                    # takes models of that block only -- the opposite
            assert np.array_equal(perm // (B // 8), xcd), t                        # order of the second target stays inside the XCD


@pytest.mark.parametrize("B", ORDER_SHAPES)
@pytest.mark.parametrize("nt", [2, 1])
def test_the_order_is_a_permutation_inside_the_xcd_blocks(eng, B, nt):
    models = synth_models(np.random.RandomState(6100 + B + nt), B, L, lvz_frac=0.1)
    try:
        if nt != 2:
            eng.set_targets(spec(nt))
        evaluate(eng, models)
        check_order(eng, B, nt, models[0])
    finally:
        if nt != 2:
            eng.set_targets(spec(2))


@pytest.mark.parametrize("nt", [2, 1])
def test_the_order_of_mixed_depths_is_a_permutation_deepest_first(eng, nt):
    Lm = 21
    models = prior_models(np.random.RandomState(78), 4096, Lm)
    try:
        if nt != 2:
            eng.set_targets(spec(nt))
        evaluate(eng, models, Lm)
        check_order(eng, 4096, nt, models[0])
    finally:
        if nt != 2:
            eng.set_targets(spec(2))


@pytest.mark.parametrize("nt", [2, 1])
def test_a_batch_beyond_the_sorted_list_takes_the_depth_order(eng, nt):
    """B above PAIR_MAX_B (12 288 models, swd_kernel.hip): no order by length, no prologue; same bits as given"""
    B = 12352
    models = synth_models(np.random.RandomState(6200 + nt), B, L, lvz_frac=0.1)
    try:
        if nt != 2:
            eng.set_targets(spec(nt))
        got = evaluate(eng, models)
        assert eng.last_swd_order() == ("depth", 1, set()) and acts(eng) == 0
        perm = eng.last_swd_perm(0, B)
        assert np.array_equal(np.sort(perm), np.arange(B))
        eng.set_model_order(sort_by_depth=False)
        assert same_bits(got, evaluate(eng, models))
    finally:
        eng.set_model_order(sort_by_depth=True)
        if nt != 2:
            eng.set_targets(spec(2))


STEADY = (0, 7, 8, 9, 10, 11, 14, 15)  # counters that depend neither on time nor on which models share a wavefront


def dirty_and_clean(B):
    """a batch that leaves something in every word the ordering launch zeroes -- models from a sampler's prior (the guard lists
    some) with one insane model (a failure flag) -- and a batch of the same shape that must see none of it"""
    dirty = tuple(a.copy() for a in prior_models(np.random.RandomState(11), max(B, 64), L))
    dirty = tuple(np.ascontiguousarray(a[..., :B]) for a in dirty)
    dirty[2][:, B // 2] = 200.0  # vp
    return dirty, synth_models(np.random.RandomState(12), B, L, lvz_frac=0.1)


def one_call(e, models):
    out = evaluate(e, models)
    c = e.debug_counters()
    e.last_neval()  # (the next call's counters start from zero)
    return dict(out=out, guard=e.guard_stats()[0], fills=e.last_swd_order()[2], order=e.last_swd_order()[0], counters=[c[i] for i in STEADY])


@pytest.mark.parametrize("B", [1, 5, 32, 33, 67, 1024, 1032])
def test_the_fills_still_happen(eng, B):
    """guard words, failure flags and counters are zero when the dispersion kernel starts: after a call that left counts, flags and
    counters behind, a clean batch of the same shape gives what a fresh engine gives -- outputs, guard counts, counters"""
    dirty, clean = dirty_and_clean(B)
    f = E.Engine(0)
    try:
        f.set_swd_trials(TRIALS)
        f.set_targets(spec(2))
        f.set_instrumentation(timing=False, counting=True)
        fresh = one_call(f, clean)
    finally:
        f.close()
    eng.set_instrumentation(timing=False, counting=True)
    try:
        first = one_call(eng, dirty)
        again = one_call(eng, clean)
    finally:
        eng.set_instrumentation(timing=False, counting=False)
    assert first["out"][2][B // 2] != 0                                  # the dirty call did leave a flag
    if B > 1:                                                            # the ordering launch is the call's prologue
        assert again["order"] == "length" and {"guard", "counters"} <= again["fills"] and "flags" in fresh["fills"]
    else:
        assert again["order"] == "none" and again["fills"] == set()
    assert again["out"][2][B // 2] == fresh["out"][2][B // 2]             # ... which the next call does not see
    assert same_bits(again["out"], fresh["out"]) and again["guard"] == fresh["guard"] and again["counters"] == fresh["counters"]


def test_the_sampler_walks_the_same_trajectory_in_the_order_as_given():
    """8 chains, two iterations per evaluation launch, 50 iterations: the chain state with the engine's own order and with the
    order as given"""
    from conftest import golden
    from bayhunter_amd.device_chains import DeviceChains
    from test_gpu_chains import SETUPS, make_targets
    g = golden("chain_golden.npz")
    su = SETUPS["exp"]
    init = dict(su["init"], iter_burnin=30, iter_main=20, maxmodels=25)
    keys = ("n", "vs", "z", "like", "noise", "vpvs", "misfits", "propdist", "proposed", "accepted", "naccepted")
    states = []
    for as_given in (False, True):
        dc = DeviceChains(make_targets(g), 8, init, su["priors"], seed=20261019, spec_depth=2)
        try:
            dc.engine.set_model_order(sort_by_depth=not as_given)
            states.append(dc.run().state_host())
        finally:
            dc.engine.set_model_order(sort_by_depth=True)
    assert states[0]["accepted"].sum() > 0
    for k in keys:
        assert np.array_equal(states[0][k], states[1][k]), k
