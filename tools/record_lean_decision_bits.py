#!/usr/bin/env python3
"""Record tests/golden/lean_decision_bits.npz: what the ROUND DECISIONS of the trial-per-lane dispersion kernel (csrc/swd_lean.hip:
the round loop outside the secular evaluations) lead to, with the library of the tree this script runs in -- inputs and outputs
together, so that tests/test_gpu_lean_decision_bits.py never draws an input again.  Run it ONCE, on the GPU, from the commit whose
search is the contract (the parent of a change that claims to keep it):

    python tools/record_lean_decision_bits.py [--out FILE]

The test imports compute() from here: the golden and the test make the same calls.  Single-target searches at 16 and 32 trials are
tests/golden/lean_eval_bits.npz's; here is what only the decision stage can get wrong.

Every call is the FUSED one (two targets, Rayleigh + Love phase velocities, engine defaults, evaluate_batch), with the trial count
pinned, once with the plain build and once with the counting build:

  * synth  96 of synth_models' ten-layer models, 30 periods, 16 trials
  * prior  256 of prior_models' models (2 ... 21 layers, vs 2-5, z 0-60, vpvs 1.4-2.1, thickmin 0.1: bench.py's c2p draw), 30
           periods, 16 trials -- and, counting build, 4, 8, 32 and 64 trials (4 trials: the set's models of at most 16 layers in
           arrays of 16 rows -- sixteen models of 21 rows do not fit a wavefront's share of the LDS, and the engine would take
           another kernel)
  * odd    B = 13 (not a multiple of a 16-lane wavefront's four models): ordinary models with a water-layer model and a model with
           a value that is not a number in the first wavefront, 30 periods; the same batch at ONE period; 16 trials
  * c2     bench.py's headline shape once: 4096 synthetic ten-layer models, 30 periods -- the only shape at which the engine sets
           the priority schedule and the pairing of the SIMDs' wavefronts (swd_lean_kernel<16, ., true>).  Its models are drawn
           from the seed again (a digest of them is kept); of its velocities a SHA-256 per target and the first and last 32 rows.

Kept per call: the velocities as binary32 (what the kernels write; compute() asserts that nothing is lost) or their digest, the
failure flags, the guard's counts per target, the guarded models' indices per target (sorted: the list's order is the order of
the wavefronts' atomics), whether the launch carried the priority schedule; of the counting build the counter words that are
functions of the search -- evaluations per wave type (8, 9), layer steps (10, 11), sum and maximum of the wavefronts' rounds
(1, 3, 4, 6), guard reasons (14, 15) -- not the cycle words.  (Where a call has guarded models its re-run launch adds that
kernel's phase clocks to words 1 ... 6: the test compares the rounds' words of the calls without one, synth and c2.)
"""
import argparse
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PERIODS = np.linspace(2.0, 60.0, 30)
ONE_PERIOD = np.array([11.0])
WORDS = (1, 3, 4, 6, 8, 9, 10, 11, 14, 15)  # of bh_debug_counters: functions of the search, not of timing
OTHER_TRIALS = (4, 8, 32, 64)
ROWS_4 = 16  # rows of the model arrays of the call with 4 trials
C2_SEED, C2_B, C2_ROWS = 4723, 4096, 32


def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8).copy()


def c2_models():
    from bayhunter_amd.synth import synth_models
    nlay, h, vp, vs, rho = synth_models(np.random.RandomState(C2_SEED), C2_B, 10, lvz_frac=0.1)
    return nlay, np.stack([h, vp, vs, rho]).astype(np.float32)


def build_inputs():
    """the inputs of every recorded call, as the arrays the file keeps"""
    from bayhunter_amd.synth import prior_models, synth_models

    d = {"periods": PERIODS, "one_period": ONE_PERIOD}
    rs = np.random.RandomState(4721)
    nlay, h, vp, vs, rho = synth_models(rs, 96, 10, lvz_frac=0.1)
    d["synth_nlay"], d["synth_model"] = nlay, np.stack([h, vp, vs, rho]).astype(np.float32)
    nlay, h, vp, vs, rho = prior_models(rs, 256, 21, vs=(2.0, 5.0), z=(0.0, 60.0), vpvs=(1.4, 2.1), thickmin=0.1)
    d["prior_nlay"], d["prior_model"] = nlay, np.stack([h, vp, vs, rho]).astype(np.float32)
    nlay, h, vp, vs, rho = synth_models(np.random.RandomState(4722), 13, 10, lvz_frac=0.1)
    m = np.stack([h, vp, vs, rho]).astype(np.float32)
    m[2, 0, 1] = 0.0      # model 1: a water layer on top
    m[2, 3, 2] = np.nan   # model 2: a value that is not a number
    d["odd_nlay"], d["odd_model"] = nlay, m
    d["c2_model_sha"] = _sha(c2_models()[1])
    return d


def fused(engine, nlay, model, periods, trials, counting):
    """one fused call of Rayleigh + Love phase velocities: {velocities [2][B, K] binary32, flags, guard counts, guard lists, schedule, counters}"""
    from bayhunter_amd import engine as E
    h, vp, vs, rho = (x.astype(np.float64) for x in model)
    B, K = int(nlay.size), int(periods.size)
    yobs = 3.4 + 0.01 * periods
    engine.set_instrumentation(False, bool(counting))
    engine.set_targets([dict(kind=E.TARGET_SWD, law=E.LAW_NOCORR, n=K, x=periods, yobs=yobs, iwave=2, igr=0),
                        dict(kind=E.TARGET_SWD, law=E.LAW_NOCORR, n=K, x=periods, yobs=yobs, iwave=1, igr=0)])
    noise = np.tile([0.0, 0.05, 0.0, 0.05], (B, 1))
    with engine.trying(trials):
        _, _, err, ymod = engine.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True)
        assert engine.last_swd_kernel() == "lean"
        main = [l for l in engine.last_swd_launches() if l["family"] == "lean" and l["role"] == "main"]
        assert len(main) == 1 and main[0]["key"][0] == trials and bool(main[0]["key"][1]) == bool(counting), main
        counts = engine.guard_stats()[0][:2]
        lists = [np.sort(engine.guard_list(t, B)) for t in range(2)]
        words = engine.debug_counters() if counting else None
    engine.set_instrumentation(False, False)
    v32 = ymod.astype(np.float32)
    assert np.array_equal(ymod, v32.astype(np.float64), equal_nan=True), "velocities are binary32 values"
    out = {"vel_r": v32[:, :K], "vel_l": v32[:, K:2 * K], "err": err.astype(np.int8), "guard": np.array(counts, dtype=np.int64),
           "glist_r": lists[0].astype(np.int32), "glist_l": lists[1].astype(np.int32), "sched": np.array([main[0]["fair"] != 0], dtype=np.int8)}
    if counting:
        out["words"] = np.array([words[i] for i in WORDS], dtype=np.uint64)
    return out


def compute(engine, d):
    """{name: array}: every output the file keeps, from the inputs d, with `engine` (left on the default search and arithmetic)"""
    engine.set_swd_search("fast")
    engine.set_swd_arith("fast")
    out = {}

    def keep(tag, r, digest=False):
        for k, v in r.items():
            if digest and k.startswith("vel_"):
                out["%s_%s_sha" % (tag, k)] = _sha(v)
            else:
                out["%s_%s" % (tag, k)] = v

    for pop, per in (("synth", "periods"), ("prior", "periods"), ("odd", "periods"), ("odd", "one_period")):
        tag = pop if per == "periods" else pop + "1"
        for counting in (False, True):
            keep("%s_t16_%s" % (tag, "cnt" if counting else "run"), fused(engine, d[pop + "_nlay"], d[pop + "_model"], d[per], 16, counting))
    for trials in OTHER_TRIALS:
        nlay, model = d["prior_nlay"], d["prior_model"]
        if trials == 4:
            sel = nlay <= ROWS_4
            nlay, model = nlay[sel], np.ascontiguousarray(model[:, :ROWS_4, sel])
        keep("prior_t%d_cnt" % trials, fused(engine, nlay, model, d["periods"], trials, True), digest=True)
    nlay, model = c2_models()
    assert np.array_equal(_sha(model), d["c2_model_sha"]), "the c2 models are not the recorded draw"
    for counting in (False, True):
        r = fused(engine, nlay, model, d["periods"], 16, counting)
        tag = "c2_t16_%s" % ("cnt" if counting else "run")
        for w in ("r", "l"):
            v = r["vel_" + w]
            out["%s_vel_%s_head" % (tag, w)], out["%s_vel_%s_tail" % (tag, w)] = v[:C2_ROWS].copy(), v[-C2_ROWS:].copy()
        keep(tag, r, digest=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "lean_decision_bits.npz"))
    a = ap.parse_args()
    from bayhunter_amd import engine as E

    eng = E.Engine(0)
    d = build_inputs()
    d.update(compute(eng, d))
    np.savez_compressed(a.out, **d)
    print("%s: %d arrays, %d bytes" % (a.out, len(d), os.path.getsize(a.out)))
    for k in sorted(d):
        if k.endswith("_guard"):
            t = k[:-6]
            print("  %-18s failed %4d  guard %s  schedule %d  %s" % (t, int((d[t + "_err"] != 0).sum()), d[k].tolist(), int(d[t + "_sched"][0]),
                                                                    ("words " + str(d[t + "_words"].tolist())) if t + "_words" in d else ""))


if __name__ == "__main__":
    main()
