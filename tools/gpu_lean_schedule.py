#!/usr/bin/env python3
"""What an order of the models is worth to the trial-per-lane dispersion launch, MEASURED: the c2 batch of bench.py (its seed, first batch
of the pool) run in the device's own order and, through set_model_order(False), in orders made on the host -- the parent's key restated,
the order as generated, and the orders of keys no ordering launch can have (the counted rounds of tools/cpu_lean_schedule.py): the upper
bound of what any key can give.  Per order: the dispersion family's time per call (untraced build, the orders taken in turn), then one call
of the counting build, whose per-wavefront records (rounds, cycles, SIMD) give the longest and the mean SIMD and which wavefronts share one.
Dev tool.
    python tools/gpu_lean_schedule.py [out_prefix] [calls per turn] [turns]"""
import sys, os, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import cpu_lean_schedule as S
from bayhunter_amd import engine as E
from bayhunter_amd.synth import synth_models, SWD_PERIODS, SEED

prefix = sys.argv[1] if len(sys.argv) > 1 else "lean_schedule"
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 50
TURNS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
B = 4096
nlay, h, vp, vs, rho = synth_models(np.random.RandomState(SEED), B, 10, lvz_frac=0.1)
RR, _ = S.counted_rounds(nlay, h, vp, vs, rho, SWD_PERIODS, 2)
RL, _ = S.counted_rounds(nlay, h, vp, vs, rho, SWD_PERIODS, 1, love_skip=not os.environ.get("BH_SWD_LEAN_NO_SKIP"))  # (as the kernel runs them)


def host_perm(key):
    """the batch order in which wavefront `wid` of the as-given launch gets the group the blocked ordering launch would hand it"""
    sb = S.block_sort(key)
    per = B // S.BLOCKS
    p = np.zeros(B, np.int64)
    for x in range(S.BLOCKS):
        for q in range(per // S.MPW):
            wid = ((q >> 1) << 4) | (x << 1) | (q & 1)
            p[wid * S.MPW:(wid + 1) * S.MPW] = sb[x][q * S.MPW:(q + 1) * S.MPW]
    return p


walk_steps, walk_rounds = S.key_walk(nlay, h, vs, SWD_PERIODS)
PLAIN = "device, as dispatched: no priorities, plain opposite order"
orders = {
    "device": None,
    PLAIN: None,
    "host: range of vs (the parent's key restated)": host_perm(S.key_range(nlay, h, vs)),
    "host: as generated": np.arange(B),
    "host: counted Rayleigh rounds": host_perm(RR.astype(np.float32)),
    "host: counted 22.6 R + 17.0 L": host_perm((S.KCYC_R * RR + S.KCYC_L * RL).astype(np.float32)),
    "host: counted Love rounds": host_perm(RL.astype(np.float32)),
    "host: predicted walk, steps": host_perm(walk_steps),
    "host: predicted walk, rounds": host_perm(walk_rounds),
}
eng = E.Engine(0)
yobs = 3.4 + 0.01 * SWD_PERIODS
eng.set_targets([dict(kind=E.TARGET_SWD, law=0, n=30, x=SWD_PERIODS, yobs=yobs, iwave=2, igr=0),
                 dict(kind=E.TARGET_SWD, law=0, n=30, x=SWD_PERIODS, yobs=yobs, iwave=1, igr=0)])
noise = np.tile([0, 0.05, 0, 0.05], (B, 1))
SHARE = eng.tuning("swd_lean_share")


def run(p, n, k=None):
    for name, v in (("swd_lean_share", 0), ("swd_lean_no_half", 1)) if k == PLAIN else (("swd_lean_share", SHARE), ("swd_lean_no_half", 0)):
        eng.set_tuning(name, v)
    eng.set_model_order(p is None)
    a = (nlay, h, vp, vs) if p is None else (nlay[p], np.ascontiguousarray(h[:, p]), np.ascontiguousarray(vp[:, p]), np.ascontiguousarray(vs[:, p]))
    out = None
    for _ in range(n):
        out = eng.evaluate_batch(*a, noise)
    if p is not None:  # back to the batch's own order
        inv = np.argsort(p)
        out = tuple(o[inv] for o in out)
    return out


ref = None
times = {k: [] for k in orders}
eng.set_instrumentation(True, False)
for k, p in orders.items():  # warm-up, and: every order gives the same bits
    out = run(p, 2, k)
    if ref is None:
        ref = out
    same = all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(ref, out))
    print("%-48s same bits as the device's order: %s" % (k, same), flush=True)
    assert same
for turn in range(TURNS):
    for k, p in orders.items():
        run(p, 1, k)
        eng.timing_reset()
        run(p, CALLS, k)
        n, tot, fam = eng.timing_collect()
        times[k].append(fam["swd"] / n)
print("dispersion family, ms per call (%d turns of %d calls): min / median / max" % (TURNS, CALLS))
for k, v in times.items():
    print("  %-48s %.4f / %.4f / %.4f" % (k, min(v), float(np.median(v)), max(v)), flush=True)

report = {"ms_per_call": times, "trace": {}}
for k, p in orders.items():
    eng.set_instrumentation(True, True)
    run(p, 1, k)
    eng.timing_reset()
    run(p, 1, k)
    eng.timing_collect()
    c = eng.debug_counters()
    tr = eng.debug_trace()
    eng.set_instrumentation(True, False)
    cyc = (tr[:, 2] & 0xffffffffff).astype(float)
    gwid = (tr[:, 2] >> 40).astype(np.int64)
    rounds = (tr[:, 3] & 0xffffffff).astype(int)
    ifn = ((tr[:, 3] >> 32) & 0xf).astype(int)
    hw = (tr[:, 3] >> 36).astype(np.int64)
    t0 = tr[:, 0].min()
    start, end = (tr[:, 0] - t0) / 100.0, (tr[:, 1] - t0) / 100.0
    key = (((hw >> 8) & 0xfff) << 2) | ((hw >> 4) & 3)  # (xcc, se, sh, cu, simd)
    np.save("%s_trace_%d.npy" % (prefix, list(orders).index(k)), np.column_stack((gwid, key, ifn, rounds, cyc, start, end)))
    u, inv = np.unique(key, return_inverse=True)
    simd_end = np.zeros(u.size); np.maximum.at(simd_end, inv, end)
    simd_start = np.full(u.size, 1e30); np.minimum.at(simd_start, inv, start)
    nR = np.bincount(inv, ifn == 2, u.size); nL = np.bincount(inv, ifn == 1, u.size)
    busy = simd_end - simd_start
    rec = dict(simds=int(u.size), simds_one_R_one_L=int(((nR == 1) & (nL == 1)).sum()), longest_simd_us=float(busy.max()), mean_simd_us=float(busy.mean()),
               span_us=float(end.max()), rounds_R_mean=float(rounds[ifn == 2].mean()), rounds_R_max=int(rounds[ifn == 2].max()),
               rounds_L_mean=float(rounds[ifn == 1].mean()), rounds_L_max=int(rounds[ifn == 1].max()),
               kcyc_per_round_R=float(np.median(cyc[ifn == 2] / rounds[ifn == 2]) / 1e3), kcyc_per_round_L=float(np.median(cyc[ifn == 1] / rounds[ifn == 1]) / 1e3))
    # the two wavefronts of a SIMD by age: the workgroup of the first pass is the older
    gmin = np.full(u.size, 1 << 40); np.minimum.at(gmin, inv, gwid)
    isR = ifn == 2
    r_first = np.zeros(u.size, bool); r_first[inv[isR & (gwid == gmin[inv])]] = True
    dur = end - start
    for nm, m in (("Rayleigh older", r_first), ("Love older", ~r_first)):
        sel = m[inv]
        rec[nm] = dict(simds=int(m.sum()), end_mean_us=float(simd_end[m].mean()), end_max_us=float(simd_end[m].max()),
                       R_us=float(dur[sel & isR].mean()), L_us=float(dur[sel & ~isR].mean()), R_rounds=float(rounds[sel & isR].mean()), L_rounds=float(rounds[sel & ~isR].mean()))
    if p is None:  # the device's own order, read back: counted against actual rounds, wavefront by wavefront
        perm, Q, H = eng.last_swd_perm(0, B), B // S.MPW // 8, 0 if k == PLAIN else B // S.MPW // 16
        ty, wid = gwid & 1, gwid >> 1  # two targets of equal wavefront counts: interleaved one by one (swd_lean_kernel)
        x, q = (wid >> 1) & 7, ((wid >> 4) << 1) | (wid & 1)
        qr = np.where(ty == 1, np.array([S.love_group(int(v), Q, H) for v in q]), q)
        grp = ((qr >> 1) << 4) + 2 * x + (qr & 1)
        counted = np.where(ty == 1, RL[perm].reshape(-1, S.MPW).max(1)[grp], RR[perm].reshape(-1, S.MPW).max(1)[grp])
        for nm, m in (("Rayleigh", ty == 0), ("Love", ty == 1)):
            assert np.all((ifn[m] == 2) == (nm == "Rayleigh"))
            d = rounds[m] - counted[m]
            rec["counted_vs_actual_" + nm] = dict(corr=float(np.corrcoef(counted[m], rounds[m])[0, 1]), mean_diff=float(d.mean()), max_diff=int(d.max()), min_diff=int(d.min()),
                                                  equal=float((d == 0).mean()))
            print("    %-8s wavefronts: rounds counted on the CPU against rounds taken: correlation %.3f, taken - counted mean %.2f (min %d, max %d), equal on %.2f" % (
                nm, rec["counted_vs_actual_" + nm]["corr"], d.mean(), d.min(), d.max(), (d == 0).mean()))
    report["trace"][k] = rec
    print("%-48s SIMDs %d (one R + one L: %d)  longest %.1f us, mean %.1f us, ratio %.3f; span %.1f us" % (k, rec["simds"], rec["simds_one_R_one_L"], rec["longest_simd_us"], rec["mean_simd_us"], rec["longest_simd_us"] / rec["mean_simd_us"], rec["span_us"]))
    for nm in ("Rayleigh older", "Love older"):
        print("    SIMDs with the %-14s wavefront (%d): end mean %.1f max %.1f us; Rayleigh wavefront %.1f us for %.1f rounds, Love %.1f us for %.1f rounds" % (
            nm, rec[nm]["simds"], rec[nm]["end_mean_us"], rec[nm]["end_max_us"], rec[nm]["R_us"], rec[nm]["R_rounds"], rec[nm]["L_us"], rec[nm]["L_rounds"]))
    print("    rounds R mean %.1f max %d, L mean %.1f max %d; kcycles per round R %.1f L %.1f" % (rec["rounds_R_mean"], rec["rounds_R_max"], rec["rounds_L_mean"], rec["rounds_L_max"], rec["kcyc_per_round_R"], rec["kcyc_per_round_L"]), flush=True)
with open(prefix + ".json", "w") as f:
    json.dump(report, f, indent=1)
