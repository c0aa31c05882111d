"""The launch in front of the dispersion kernel: it orders the models (csrc/swd_kernel.hip: pair_order_blocked_kernel, a workgroup
per XCD block of a blocked order; pair_order_kernel, one workgroup, for every other batch) and, as the call's prologue, zeroes
the words that had fill dispatches of their own before (the guard's head, the failure flags, the counters: SwdFills).

Neither may show in a result.  An order is scheduling only, so every order gives the same BITS; and a call's outputs, guard
counts and counters are what a fresh engine gives for it, whatever the calls before it left in the work words.

c2's targets (Rayleigh and Love phase velocities at 30 periods) on an engine of its own with the default search and
arithmetic, the trials of the trial-per-lane kernel pinned to 16 -- a model's velocities depend on that number and on nothing
else about the call (include/bh_engine_debug.h), so a model evaluated alone must give the bits it gives inside a batch."""
import numpy as np
import pytest

from bayhunter_amd import engine as E
from bayhunter_amd.synth import synth_models, prior_models, SWD_PERIODS

pytestmark = pytest.mark.gpu
L = 10
TRIALS = 16     # 4 models per wavefront


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


def evaluate(e, models):
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
    e.evaluate_batch_dev(B, L, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), B, 1,
                         d_noise.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), ymod=out[3].data_ptr(),
                         stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def same_bits(a, b):
    return all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def take(models, idx):
    return tuple(np.ascontiguousarray(a[..., idx]) for a in models)


# (models, ragged, targets) -> the order the plan takes and the workgroups of its launch.  16 trials = 4 models per wavefront;
# blocked = the wavefronts of a target divide over 8 XCDs x the wavefronts of that target per workgroup (2 with two targets, 4 with one).
SHAPES = [
    (1, False, 2, "none", 0),          # nothing to order
    (5, False, 2, "length", 1),        # not a whole wavefront
    (64, False, 2, "length", 8),       # the smallest blocked batch: 16 wavefronts per target, 8 models per block
    (1024, False, 2, "length", 8),     # 256 wavefronts per target, blocks of 128
    (520, False, 2, "length", 1),      # 130 wavefronts: not divisible
    (256, True, 2, "length", 8),       # mixed depths of 2 .. 10 layers: one order over the batch, deepest first, the eight
    #                                    workgroups each placing their block's models in it
    (8704, False, 2, "length", 8),     # blocks of 1088: two models per thread
    (8704, True, 2, "length", 8),
    (12352, False, 2, "depth", 1),     # beyond the 12 288 models the sort holds: order_kernel, the call fills for itself
    (12352, False, 1, "depth", 1),
]


@pytest.mark.parametrize("B,ragged,nt,order,wgs", SHAPES)
def test_every_order_gives_the_same_bits(eng, B, ragged, nt, order, wgs):
    models = synth_models(np.random.RandomState(4100 + B + nt), B, L, lvz_frac=0.1, ragged=ragged)
    try:
        if nt != 2:
            eng.set_targets(spec(nt))
        got = evaluate(eng, models)
        assert eng.last_swd_kernel() == "lean"
        launches = eng.last_swd_launches()
        assert [(r["family"], r["role"]) for r in launches] == [("lean", "main"), ("group", "rerun")]
        assert launches[0]["key"][0] == TRIALS and launches[0]["interleaved"] == (nt == 2)
        o, w, fills = eng.last_swd_order()
        assert (o, w) == (order, wgs)
        # the launch of an order by length is the call's prologue: it zeroes the guard's head; the other calls fill for themselves
        assert ("guard" in fills) == (order == "length") and (order == "length" or not fills)
        assert np.all(got[2] >= 0) and np.isfinite(got[0][got[2] == 0]).all()
        eng.set_model_order(sort_by_depth=False)
        as_given = evaluate(eng, models)
        assert eng.last_swd_order() == ("none", 0, set()) and eng.last_swd_kernel() == "lean"
        assert same_bits(got, as_given)
        for b in np.unique(np.linspace(0, B - 1, 8).astype(int)):       # 8 models of the batch, each alone
            alone = evaluate(eng, take(models, [b]))
            assert same_bits(alone, [a[[b]] for a in got]), b
    finally:
        eng.set_model_order(sort_by_depth=True)
        if nt != 2:
            eng.set_targets(spec(2))


GUARDED_SEED, CLEAN_SEED = 11, 12     # (batches chosen on the commit before the prologue: the first guards models, the second none)
STEADY = (0, 7, 8, 9, 10, 11, 14, 15)  # the counters that depend neither on time nor on which models share a wavefront:
#                                        evaluations, wavefronts, evaluations and layer steps per wave type, guard reasons


def four_batches():
    """a batch from the chains' prior (ragged, velocities in any order: the guard fires on some), c2 models the guard leaves
    alone, the same with one insane model, and the same again"""
    guarded = prior_models(np.random.RandomState(GUARDED_SEED), 64, L)
    clean = synth_models(np.random.RandomState(CLEAN_SEED), 64, L, lvz_frac=0.1)
    insane = tuple(a.copy() for a in clean)
    insane[2][:, 37] = 200.0           # vp
    return guarded, clean, insane, clean


def calls(e, batches, counting):
    """One call per batch on engine e: its outputs, the guard's per-call counts, the order's record and, where the engine counts,
    the steady counters of the call"""
    rec = []
    for models in batches:
        out = evaluate(e, models)
        counters = None
        if counting:
            c = e.debug_counters()
            e.last_neval()             # (the next call's counters start from zero)
            counters = [c[i] for i in STEADY]
        rec.append(dict(out=out, guard=e.guard_stats()[0], order=e.last_swd_order(), counters=counters))
    return rec


@pytest.mark.parametrize("counting", [False, True])
def test_a_call_starts_from_zeroed_words_whatever_the_call_before_left(eng, counting):
    batches = four_batches()
    fresh = []
    for models in batches:                      # what a fresh engine gives for each call
        f = E.Engine(0)
        f.set_swd_trials(TRIALS)
        f.set_targets(spec(2))
        f.set_instrumentation(timing=False, counting=counting)
        fresh += calls(f, [models], counting)
        f.close()
    eng.set_instrumentation(timing=False, counting=counting)
    try:
        rec = calls(eng, batches, counting)
    finally:
        eng.set_instrumentation(timing=False, counting=False)
    want = {"guard", "counters"} if counting else {"guard"}
    for k, (r, f) in enumerate(zip(rec, fresh)):
        # a blocked order: the launch of eight workgroups zeroes the guard's head and the counters on every call, the failure
        # flags on the first call of a layout
        assert r["order"][:2] == f["order"][:2] == ("length", 8), k
        assert f["order"][2] == want | {"flags"} and r["order"][2] - {"flags"} == want, k
        assert k == 0 or r["order"][2] == want, k
        assert same_bits(r["out"], f["out"]), k
        assert r["guard"] == f["guard"], k
        assert r["counters"] == f["counters"] and (r["counters"] is not None) == counting, k
    assert sum(rec[0]["guard"]) > 0                                   # the first batch does leave counts in the guard's head
    assert rec[1]["guard"] == [0] * 8 and not rec[1]["out"][2].any()  # ... the second call sees none of them, and no flag
    assert rec[2]["out"][2][37] != 0 and np.count_nonzero(rec[2]["out"][2]) == 1
    assert not rec[3]["out"][2].any() and same_bits(rec[3]["out"], rec[1]["out"])
