#!/usr/bin/env python3
"""Record tests/golden/lean_eval_bits.npz: what the fast arithmetic of the dispersion kernels (csrc/swd_fa.h, csrc/swd_lean.hip)
returns, BIT FOR BIT, with the library of the tree this script runs in -- inputs and outputs together, so that
tests/test_gpu_lean_eval_bits.py never draws an input again.  Run it ONCE, on the GPU, from the commit whose bits are the
contract (the parent of a change that claims to keep them):

    python tools/record_lean_eval_bits.py [--out FILE]

The test imports compute() from here: the golden and the test make the same calls.

  * fn_*: the functions of namespace fa (bh_probe_math ops 17-23).  rcp, rcp1, sqrt_rsqrt: one set of positive inputs.  sincos:
    0, 9e4, multiples of pi/4 and their neighbours one unit in the last place away, a uniform sample.  expneg: 0, 700, subnormal
    and tiny x, x = k ln 2 / 2 for odd k (where rint switches n) and its neighbours, the x that give n = 0, -1, -1009, -1010, a
    uniform sample of [0, 700].
  * sec_*: the secular functions (bh_probe_swd_secular, evaluators 1 and 2, Love and Rayleigh) of models of 2, 3, 10, 11 and 32
    layers -- odd and even counts: the lean evaluator's normalisation keys on the layer's parity -- and of a model with a layer
    thick enough to poison, each with mtop = mmax and mtop = mmax + 1 (one NaN row of ragged filler; evaluator 2 has rows for 32
    layers, so its 32-layer model has no second case), at 64 points: tests/swd_fa_ref.py's points (uniform, within
    1e-6 ... 1e-12 of layer and half-space velocities on both sides), four of the uniform ones replaced by k == k_beta exactly.
  * run_*: whole searches, swd_batch with the engine's default search and arithmetic, trials pinned to 16 and to 32: 256 of
    synth_models' ten-layer models (lvz_frac 0.1) and 256 of prior_models' ragged 2 ... 20-layer models, Rayleigh and Love,
    eight periods.  Models are stored as binary32 (the kernels read them as that), velocities as binary32 (what they write).

Sizes are what keeps the file under 300 KB; every kind of input above is present at each size.
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

OPS = {"rcp": 17, "rcp1": 18, "sqrt": 19, "rsqrt": 20, "sin": 21, "cos": 22, "expneg": 23}
SEC_LAYERS = (2, 3, 10, 11, 32)
LEAN_ROWS = 32  # rows of evaluator 2's model (csrc/swd_lean.hip: PROBE_LEAN_ROWS)
TRIALS = (16, 32)
PERIODS = np.linspace(2.0, 60.0, 8)
LN2 = 0.6931471805599453


def _near(x):
    """x and its two neighbours"""
    x = np.asarray(x, dtype=np.float64)
    return np.concatenate([x, np.nextafter(x, np.inf), np.nextafter(x, -np.inf)])


def build_inputs():
    """the inputs of every recorded call, as the arrays the file keeps"""
    import swd_fa_ref as R
    from bayhunter_amd.synth import prior_models, synth_models

    d = {}
    rs = np.random.RandomState(4711)
    d["fn_pos_x"] = np.concatenate([10.0 ** rs.uniform(-3, 3, 184), rs.uniform(0.5, 2.0, 64), [1.0, 2.0, 0.5, 3.0, 1.0e-290, 1.0e290, 4.0, 0.25]])
    q = np.unique(np.concatenate([np.arange(1, 161), rs.randint(161, 114591, 200), [114590, 114591]])).astype(np.float64) * (np.pi / 4)
    x = np.concatenate([[0.0, 9.0e4], _near(q), rs.uniform(0, 10, 300), rs.uniform(0, 9.0e4, 500)])
    d["fn_sincos_x"] = x[(x >= 0.0) & (x <= 9.0e4)]
    kodd = np.unique(np.concatenate([np.arange(1, 100, 2), np.arange(101, 2019, 16), [2015, 2017, 2019]])).astype(np.float64)
    nedge = np.array([0.0, 1.0, 1009.0, 1010.0]) * LN2  # n = 0, -1, -1009, -1010 (and, beside them, what their neighbours give)
    x = np.concatenate([[0.0, 700.0, 5.0e-324, 2.0e-308, 1.0e-300, 1.0e-100, 1.0e-17, 1.0e-8], _near(kodd * (LN2 / 2)), _near(nedge),
                        nedge + 0.1, rs.uniform(0, 3, 300), rs.uniform(0, 700, 900)])
    d["fn_expneg_x"] = x[(x >= 0.0) & (x <= 700.0)]

    rs = np.random.RandomState(4712)
    models = [("lvz%d" % n, R.lvz_model(rs, n)) for n in SEC_LAYERS]
    dd = np.array([2.0, 2.0e6, 5.0, 0.0], dtype=np.float32)  # (tests/test_gpu_swd_fa.py: test_poison_rule's model)
    vs = np.array([3.0, 3.5, 3.9, 4.5], dtype=np.float32)
    vp = (1.75 * vs).astype(np.float32)
    models.append(("thick4", (dd, vp, vs, (0.77 + 0.32 * vp).astype(np.float32))))
    d["sec_names"] = np.array([n for n, _ in models])
    for name, mdl in models:
        d["sec_%s_model" % name] = np.stack(mdl).astype(np.float32)
        for ifunc in (1, 2):
            k, om, kind, dist = R.points(rs, ifunc, mdl[0], mdl[1], mdl[2], n=64)
            # the first four (uniform) points become k == k_beta (k_alpha): filled in by limit_points() with the device's fa::rcp
            d["sec_%s_%d_k" % (name, ifunc)] = k
            d["sec_%s_%d_om" % (name, ifunc)] = om

    rs = np.random.RandomState(4713)
    nlay, h, vp, vs, rho = synth_models(rs, 256, 10, lvz_frac=0.1)
    d["run_synth_nlay"] = nlay
    d["run_synth_model"] = np.stack([h, vp, vs, rho]).astype(np.float32)
    nlay, h, vp, vs, rho = prior_models(rs, 256, 20)
    d["run_prior_nlay"] = nlay
    d["run_prior_model"] = np.stack([h, vp, vs, rho]).astype(np.float32)
    d["run_periods"] = PERIODS
    return d


def limit_points(engine, d):
    """k == k_beta exactly, as the kernels form it (omega * fa::rcp(v), one IEEE multiply): the first four points of every set"""
    for name in d["sec_names"]:
        mdl = d["sec_%s_model" % name]
        n = mdl.shape[1]
        for ifunc in (1, 2):
            k, om = d["sec_%s_%d_k" % (name, ifunc)], d["sec_%s_%d_om" % (name, ifunc)]
            v = [mdl[2][0], mdl[2][n - 1], mdl[2][n // 2], mdl[1][n // 2] if ifunc == 2 else mdl[2][(n - 1) // 2]]
            r = engine.probe_math(OPS["rcp"], np.array(v, dtype=np.float64))
            k[:4] = om[:4] * r


def compute(engine, d):
    """{name: array}: every output the file keeps, from the inputs d, with `engine` (left on the default search and arithmetic)"""
    out = {}
    for name, xs in (("rcp", "pos"), ("rcp1", "pos"), ("sqrt", "pos"), ("rsqrt", "pos"), ("sin", "sincos"), ("cos", "sincos"), ("expneg", "expneg")):
        out["fn_%s" % name] = engine.probe_math(OPS[name], d["fn_%s_x" % xs])
    for name in d["sec_names"]:
        mdl = d["sec_%s_model" % name]
        mmax = mdl.shape[1]
        rag = np.concatenate([mdl, np.full((4, 1), np.nan, dtype=np.float32)], axis=1)
        for ifunc in (1, 2):
            k, om = d["sec_%s_%d_k" % (name, ifunc)], d["sec_%s_%d_om" % (name, ifunc)]
            for ev in (1, 2):
                for tag, m in (("top", mdl), ("rag", rag)):
                    if ev == 2 and m.shape[1] > LEAN_ROWS:
                        continue
                    out["sec_%s_%d_ev%d_%s" % (name, ifunc, ev, tag)] = engine.probe_swd_secular(ev, ifunc, mmax, m[0], m[1], m[2], m[3], k, om)
    engine.set_swd_search("fast")
    engine.set_swd_arith("fast")
    per = d["run_periods"]
    for pop in ("synth", "prior"):
        nlay = d["run_%s_nlay" % pop]
        h, vp, vs, rho = (x.astype(np.float64) for x in d["run_%s_model" % pop])
        for trials in TRIALS:
            for ifunc, wave in ((2, "r"), (1, "l")):
                with engine.trying(trials):
                    before = engine.guard_stats()[1]
                    vel, err = engine.swd_batch(nlay, h, vp, vs, rho, per, ifunc, 0)
                    counts, after = engine.guard_stats()
                assert np.array_equal(vel, vel.astype(np.float32).astype(np.float64)), "velocities are binary32 values"
                key = "run_%s_%s_t%d" % (pop, wave, trials)
                out[key + "_vel"] = vel.astype(np.float32)
                out[key + "_err"] = err.astype(np.int8)
                out[key + "_guard"] = np.array(list(counts) + [after - before], dtype=np.int64)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "lean_eval_bits.npz"))
    a = ap.parse_args()
    from bayhunter_amd import engine as E

    eng = E.Engine(0)
    d = build_inputs()
    limit_points(eng, d)
    d.update(compute(eng, d))
    np.savez_compressed(a.out, **d)
    nan = sum(int(np.isnan(v).sum()) for k, v in d.items() if k.startswith("sec_") and "_ev" in k)
    print("%s: %d arrays, %d bytes; %d NaN among the secular values; guarded models per run: %s"
          % (a.out, len(d), os.path.getsize(a.out), nan, {k[4:-6]: int(v[:8].sum()) for k, v in d.items() if k.endswith("_guard")}))


if __name__ == "__main__":
    main()
