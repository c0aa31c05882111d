"""The Rayleigh ellipticity as a target of the fused call (include/bh_engine_ellip_target.h): what the call costs with the search
shared, with a search of its own, against the floor of its parts, and against the route that exists beside it.

Workload: bench.py's c2 shape -- 4096 models x 10 layers, 30 periods --, targets [Rayleigh phase, ellipticity at the same
periods], the engine's default search.  One session; every figure the best of `--repeat` (3) windows of `--inner` calls that end in
a synchronisation, with the spread (max - min) / best of the windows; the variants alternate inside every repeat, each after its
own registration (outside the window).  Device arrays unless stated.

  A  the fused call, search shared (bh_evaluate_batch on device pointers)
  B  the same with the ellipticity's last period moved by one bit: a search of its own -- the cost without sharing
  C  the fused [Rayleigh phase] call followed by bh_swd_ellip(have_vel = 1) on its velocities: the floor of the parts, without
     the second likelihood column
  D  from host arrays: JointTarget.evaluate_batch with RayleighEllipticity(fused=True) against fused=False (the route of the
     commit before, unchanged).  The bar: fused no slower than unfused by more than the spread of the unfused repeats.
  chains  DeviceChains, bare iterate() loop, chain-iterations/s: 8 chains, and 64 chains as one rung each of a ladder (sweep every
     100), for [phase, ellipticity fused] against [phase] alone.

    python tools/gpu_ellip_fused_perf.py [--out profiles/ellip_fused_perf.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/gpu_ellip_fused_perf.py --only-a     (a run of its own)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, L = 4096, 10
PRIORS = dict(vpvs=(1.4, 2.1), layers=(1, 20), vs=(2, 5), z=(0, 60), swdnoise_corr=0., swdnoise_sigma=(1e-5, 0.1),
              ellnoise_corr=0., ellnoise_sigma=(1e-3, 0.2))


def windows(eng, fn, inner, repeat):
    """seconds per call of `repeat` windows of `inner` calls"""
    out = []
    for _ in range(repeat):
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        eng.synchronize()
        out.append((time.perf_counter() - t0) / inner)
    return out


def summary(ts, scale=1e3):
    return dict(best=min(ts) * scale, repeats=[t * scale for t in ts], spread=(max(ts) - min(ts)) / min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--burnin", type=int, default=1000)
    ap.add_argument("--main", type=int, default=1000)
    ap.add_argument("--only-a", action="store_true", help="variant A alone, for a kernel trace")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import bayhunter_amd as bh
    from bayhunter_amd import engine as E
    from bayhunter_amd.device_chains import DeviceChains
    from bayhunter_amd.synth import synth_models, true_model, SWD_PERIODS, SEED
    eng = E.default_engine(0)
    dev = torch.device("cuda", eng.device)
    rs = np.random.RandomState(SEED)
    nlay, h, vp, vs, rho = synth_models(rs, B, L)
    per = np.asarray(SWD_PERIODS, dtype=float)
    K = per.size
    per_bit = per.copy()
    per_bit[-1] = np.nextafter(per[-1], 0.0)
    yd, ye = 3.4 + 0.01 * per, 0.8 + 0.0 * per
    swd = {"kind": E.TARGET_SWD, "law": E.LAW_NOCORR, "n": K, "x": per, "yobs": yd, "iwave": 2, "igr": 0}

    def ell(x):
        return {"kind": E.TARGET_USER, "law": E.LAW_NOCORR, "n": K, "yobs": ye, "x": x, "nsteps": 2, "signed": False, "ratio": "hv"}

    t = {k: torch.as_tensor(v, device=dev) for k, v in dict(nlay=nlay, h=h, vp=vp, vs=vs, rho=rho, per=per).items()}
    noise2 = torch.as_tensor(np.tile([0.0, 0.05, 0.0, 0.07], (B, 1)), device=dev)
    noise1 = torch.as_tensor(np.tile([0.0, 0.05], (B, 1)), device=dev)
    logL = torch.zeros(B, dtype=torch.float64, device=dev)
    misf = torch.zeros((B, 3), dtype=torch.float64, device=dev)
    err = torch.zeros(B, dtype=torch.int32, device=dev)
    ymod = torch.zeros((B, 2 * K), dtype=torch.float64, device=dev)
    hv = torch.zeros((B, K), dtype=torch.float64, device=dev)
    flag = torch.zeros(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    models = (t["nlay"].data_ptr(), t["h"].data_ptr(), t["vp"].data_ptr(), t["vs"].data_ptr(), t["rho"].data_ptr(), B, 1)

    def fused(noise):
        eng.evaluate_batch_dev(B, L, *models, noise.data_ptr(), logL.data_ptr(), misf.data_ptr(), err.data_ptr(), ymod=ymod.data_ptr())

    def parts():
        fused(noise1)   # (one target: ymod is [B][K], the velocities)
        eng.swd_ellip_dev(B, L, *models, K, t["per"].data_ptr(), ymod.data_ptr(), err.data_ptr(), hv.data_ptr(), flag.data_ptr(),
                          have_vel=True, nsteps=2)

    variants = {"A": ([swd, ell(per)], lambda: fused(noise2)), "B": ([swd, ell(per_bit)], lambda: fused(noise2)), "C": ([swd], parts)}
    if a.only_a:
        variants = {"A": variants["A"]}
    times = {k: [] for k in variants}
    for k, (descs, fn) in variants.items():          # code objects, workspaces
        eng.set_targets(descs)
        windows(eng, fn, 5, 1)
    for _ in range(a.repeat):
        for k, (descs, fn) in variants.items():
            eng.set_targets(descs)
            fn()
            times[k] += windows(eng, fn, a.inner, 1)
    eng._owner = None
    res = {"what": __doc__.split("\n\n")[1], "B": B, "layers": L, "periods": K, "inner": a.inner, "repeat": a.repeat, "unit": "ms per call",
           "search": eng.swd_search(), "arith": eng.swd_arith()}
    for k, ts in times.items():
        res[k] = summary(ts)
    if a.only_a:
        print(json.dumps(res))
        return 0
    res["A_over_C"] = res["A"]["best"] / res["C"]["best"]
    res["B_over_A"] = res["B"]["best"] / res["A"]["best"]
    res["B_minus_C_ms"] = res["B"]["best"] - res["C"]["best"]

    # D: host arrays, the two routes of JointTarget.evaluate_batch
    def joint(fused_):
        td = bh.RayleighDispersionPhase(per, yd)
        te = bh.RayleighEllipticity(per, ye, fused=fused_)
        td.set_noise_law("nocorr")
        te.set_noise_law("nocorr")
        return bh.JointTarget([td, te], engine=eng)

    nz = np.tile([0.0, 0.05, 0.0, 0.07], (B, 1))
    routes = {"fused": joint(True), "unfused": joint(False)}
    dt = {k: [] for k in routes}
    inner_d = max(3, a.inner // 5)
    for k, jt in routes.items():
        jt.evaluate_batch(nlay, h, vp, vs, nz, rho=rho)
    for _ in range(a.repeat):
        for k, jt in routes.items():
            jt.evaluate_batch(nlay, h, vp, vs, nz, rho=rho)   # (registers again: the other route owned the engine)
            dt[k] += windows(eng, lambda: jt.evaluate_batch(nlay, h, vp, vs, nz, rho=rho), inner_d, 1)
    res["D"] = {k: summary(v) for k, v in dt.items()}
    res["D"]["fused_over_unfused"] = res["D"]["fused"]["best"] / res["D"]["unfused"]["best"]
    res["D"]["bar"] = "fused.best <= unfused.best * (1 + unfused.spread)"
    res["D"]["bar_met"] = bool(res["D"]["fused"]["best"] <= res["D"]["unfused"]["best"] * (1.0 + res["D"]["unfused"]["spread"]))

    # chains
    m = true_model(L)
    x0 = eng.swd_batch(m[0], m[1], m[2], m[3], m[4], per, 2, 0)[0][0]
    e0 = np.abs(eng.swd_ellip(m[0], m[1], m[2], m[3], m[4], per)["hv"][0])
    nrs = np.random.RandomState(SEED + 2)
    obs_d, obs_e = x0 + nrs.normal(0, 0.012, K), e0 * (1.0 + nrs.normal(0, 0.01, K))
    init = dict(iter_burnin=a.burnin, iter_main=a.main, acceptance=(40, 45), thickmin=0.1, lvz=None, hvz=None, rcond=None, maxmodels=100)

    def chain_rate(with_ell, C):
        ts = [bh.RayleighDispersionPhase(per, obs_d)] + ([bh.RayleighEllipticity(per, obs_e, fused=True)] if with_ell else [])
        kw = dict(betas=np.full(C, 1.0), ladder=np.arange(C), swap_every=100) if C == 64 else {}
        dc = DeviceChains(bh.JointTarget(ts, engine=eng), C, init, PRIORS, seed=20260927, **kw)
        eng.synchronize()
        t0 = time.perf_counter()
        while dc.iiter < dc.iter_phase2:
            dc.iterate()
        eng.synchronize()
        return C * (a.burnin + a.main) / (time.perf_counter() - t0)

    res["chains"] = {"unit": "chain-iterations/s", "iter_burnin": a.burnin, "iter_main": a.main}
    for C in (8, 64):
        rates = {"phase+ellipticity": [], "phase": []}
        chain_rate(True, C), chain_rate(False, C)     # warm-up
        for _ in range(a.repeat):
            rates["phase+ellipticity"].append(chain_rate(True, C))
            rates["phase"].append(chain_rate(False, C))
        res["chains"]["C%d" % C] = {k: dict(best=max(v), repeats=v, spread=(max(v) - min(v)) / max(v)) for k, v in rates.items()}
        res["chains"]["C%d" % C]["ratio"] = max(rates["phase+ellipticity"]) / max(rates["phase"])
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
