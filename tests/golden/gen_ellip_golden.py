#!/usr/bin/env python3
"""Generate tests/golden/ellip_exact.npz: the Rayleigh ellipticity of models of the kind a chain proposes, to 100+ digits.

CPU only; nothing of it comes from a kernel.  Per (model, period):
  c        the phase velocity of the project's CPU oracle (oracle.swd_batch: Rayleigh, phase, mode 1, the reference's search), whose
           bits the engine's reference search returns (tests/test_gpu_swd.py);
  cstar, hvstar   the root of the exact secular function next to c and the ellipticity there (tests/ellip_exact.py), rounded to
           float64;
  hv{n}, mis{n}, cpol{n}, flag{n}   the restatement (tests/ellip_ref.py: ellip) from c with n = 0 and 2 polish steps;
  digits   the working digits at which the two exact expressions of hv agreed (ellip_exact.LADDER);
  noexact  1 where there is no exact value: the search failed (the model's err, or c <= 0), the top layer is water, c lies at or
           above the half-space's S velocity, or the exact secant left c (1 +- 1e-5).
Models: N_PRIOR of synth.prior_models (velocities in any order, at most 12 layers), N_SYNTH of synth.synth_models(ragged,
lvz_frac = 0.25), the four of ellip_ref.MODELS, the 50 km layer, a model under water and one whose search fails.

    python tests/golden/gen_ellip_golden.py [--check]     (--check: compare with the committed file, byte for byte)
"""
import io
import multiprocessing
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

import ellip_exact as X   # noqa: E402
import ellip_ref as R     # noqa: E402

SEED = 20261021
N_PRIOR, N_SYNTH, LMAX = 48, 16, 12
PERIODS = np.array([0.5, 1.0, 2.0, 4.0, 8.0, 15.0, 25.0, 40.0])
KIND_PRIOR, KIND_SYNTH, KIND_NAMED = 0, 1, 2
DEEP50 = ([50.0, 10.0, 0.0], [6.1, 6.9, 8.0], [3.5, 3.9, 4.5], [2.7, 2.95, 3.3])
PATH = os.path.join(HERE, "ellip_exact.npz")


def models():
    """-> nlay [B], h, vp, vs, rho [LMAX, B] (layer-major, float64), kind [B], names of the named ones"""
    from bayhunter_amd import synth
    cols = []
    kind = []
    nlay, h, vp, vs, rho = synth.prior_models(np.random.RandomState(SEED), N_PRIOR, LMAX)
    cols += [[a[:nlay[b], b] for a in (h, vp, vs, rho)] for b in range(N_PRIOR)]
    kind += [KIND_PRIOR] * N_PRIOR
    nlay, h, vp, vs, rho = synth.synth_models(np.random.RandomState(SEED + 1), N_SYNTH, LMAX, lvz_frac=0.25, ragged=True)
    cols += [[a[:nlay[b], b] for a in (h, vp, vs, rho)] for b in range(N_SYNTH)]
    kind += [KIND_SYNTH] * N_SYNTH
    names = list(R.MODELS) + ["deep50", "water", "noroot"]
    crust = [np.array(a) for a in R.MODELS["crust"]]
    vsb = np.array([4.8, 2.0])                           # a fast layer over a slow half-space: the search fails from 15 s on
    bad = [np.array([30.0, 0.0]), vsb * 1.75, vsb, vsb * 1.75 * 0.32 + 0.77]
    cols += [[np.array(a) for a in R.MODELS[n]] for n in R.MODELS]
    cols += [[np.array(a) for a in DEEP50],
             [np.r_[1.0, crust[0]], np.r_[1.5, crust[1]], np.r_[0.0, crust[2]], np.r_[1.03, crust[3]]],
             bad]
    kind += [KIND_NAMED] * len(names)
    B = len(cols)
    out = [np.zeros((LMAX, B)) for _ in range(4)]
    nl = np.zeros(B, dtype=np.int32)
    for b, m in enumerate(cols):
        nl[b] = len(m[0])
        for a, v in zip(out, m):
            a[:nl[b], b] = v
    return nl, out[0], out[1], out[2], out[3], np.array(kind, dtype=np.int32), names


def one_pair(job):
    model, T, c = job
    r = X.ellipticity(model, T, c)
    return None if r is None else (float(r[0]), float(r[1]), r[2])


def write_npz(path, arrays):
    """an .npz whose bytes depend on the arrays alone: fixed entry times, sorted names"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    from oracle import oracle as O
    nlay, h, vp, vs, rho, kind, names = models()
    B, K = len(nlay), PERIODS.size
    with O.swd_search(0):
        c, err, _ = O.swd_batch(nlay, h.T, vp.T, vs.T, rho.T, PERIODS, 2, 0, mode=1, flsph=0)
    out = dict(periods=PERIODS, nlay=nlay, h=h, vp=vp, vs=vs, rho=rho, kind=kind, c=c, err=err)
    rounded = [R.round_model(*[a[:nlay[b], b] for a in (h, vp, vs, rho)]) for b in range(B)]
    for n in (0, 2):
        hv, mis, cpol = np.zeros((B, K)), np.zeros((B, K)), np.zeros((B, K))
        flag = np.zeros((B, K), dtype=np.int8)
        for b in range(B):
            for k in range(K):
                if err[b] == 0 and c[b, k] > 0.0:
                    hv[b, k], mis[b, k], cpol[b, k], flag[b, k] = R.ellip(rounded[b], float(PERIODS[k]), float(c[b, k]), n)
        out.update({"hv%d" % n: hv, "mis%d" % n: mis, "cpol%d" % n: cpol, "flag%d" % n: flag})
    jobs, where = [], []
    for b in range(B):
        m = rounded[b]
        if err[b] != 0 or not m[2][0] > 0.0:
            continue
        for k in range(K):
            if c[b, k] > 0.0 and c[b, k] < m[2][-1]:
                jobs.append((X.exact_model(*m), float(PERIODS[k]), float(c[b, k])))
                where.append((b, k))
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        res = pool.map(one_pair, jobs, chunksize=4)
    cstar, hvstar = np.zeros((B, K)), np.zeros((B, K))
    noexact = np.ones((B, K), dtype=np.int8)
    digits = np.zeros((B, K), dtype=np.int16)
    for (b, k), r in zip(where, res):
        if r is not None:
            cstar[b, k], hvstar[b, k], digits[b, k] = r
            noexact[b, k] = 0
    out.update(cstar=cstar, hvstar=hvstar, noexact=noexact, digits=digits)

    ok = noexact == 0
    n_exact, n_bad, n_good = int(ok.sum()), int((out["mis2"][ok] > 1e-2).sum()), int((out["mis2"][ok] < 1e-9).sum())
    pri = ok & (kind == KIND_PRIOR)[:, None]
    print("models %d (named: %s), periods %s" % (B, ", ".join(names), PERIODS))
    print("search failed on models %s; pairs with an exact value: %d of %d" % (list(np.flatnonzero(err)), n_exact, B * K))
    print("  restated mismatch after 2 steps above 1e-2: %d;  mismatch after 2 steps below 1e-9: %d" % (n_bad, n_good))
    print("  prior-drawn pairs: %d, of them mismatch after 2 steps below 1e-9: %d, above 1e-2: %d"
          % (pri.sum(), (out["mis2"][pri] < 1e-9).sum(), (out["mis2"][pri] > 1e-2).sum()))
    assert n_exact >= 250 and n_bad >= 30 and n_good >= 200, "the set misses the counts it is there for: enlarge the draw"
    if "--check" in sys.argv[1:]:
        tmp = PATH + ".check"
        write_npz(tmp, out)
        same = open(tmp, "rb").read() == open(PATH, "rb").read()
        os.remove(tmp)
        print("the committed file is reproduced byte for byte" if same else "THE COMMITTED FILE DIFFERS")
        sys.exit(0 if same else 1)
    write_npz(PATH, out)
    print("wrote", PATH, os.path.getsize(PATH))


if __name__ == "__main__":
    main()
