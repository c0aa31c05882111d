"""The certificate behind the trial-per-lane kernel's shortened Love scan (csrc/swd_lean.hip, "LOVE'S FIRST PERIOD RESUMES ITS
SCAN NEXT TO THE SLOWEST S VELOCITY"), restated in numpy and held against the reference's Love function.

THE RULE.  vmin = the model's slowest S velocity (half-space included), cm = the first period's start value, dc = 0.005, J = lanes
per model.  The scan's rounds rebase their grid: b_1 = fma(J - 1, dc, cm), b_j+1 = fma(J, dc, b_j).  m = the largest count with
fma(2, dc, b_m) <= vmin - dc, i.e. the first TWO trials of round m + 1 still at or below vmin - dc; the search starts at
c1 = b_m in the state the scan has after m rounds.  m = 0 unless the model has at least two layers and
    dmax omega <= 4.5e4 cm                       (no layer argument q = d rb can reach the 9e4 from which a value is not a number)
    (mumin omega)^2 dc >= 1e-18 vmin^3           (a lower bound of the value at every such point is >= 1e-9 = 1000 x fa::SIGN_FLOOR)
with omega the first period's angular frequency, dmax the thickest finite layer, mumin the smallest rho vs^2.

WHAT IS ASSERTED.  On every grid point of the m skipped rounds and on the two leading trials of the resumed round, the oracle's
dltar1 (the reference's Love function, max-norm scaled per layer as the kernel's) is >= 1e-9 -- positive, a thousand floors -- and
>= the rule's own lower bound min(1, mumin omega sqrt(dc / vmin^3)) (1 - 1e-9): the derivation holds where it is used.  (n dc is
exact in binary64 for n <= 2^29 -- dc has 24 significant bits -- so `n * DC + b` in numpy IS the kernel's fused operation.)"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from bayhunter_amd.synth import synth_models, prior_models, SWD_PERIODS, SEED

f32 = np.float32
DC = float(f32(0.005))
FLOOR = 1.0e-12          # fa::SIGN_FLOOR (csrc/swd_fa.h)
MARGIN = 1.0e3           # the rule asks for a value bound of MARGIN x FLOOR
LANES = (4, 16, 64)
N = 2000                 # models per family


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def start_value(O, a, b):
    """cm of the kernel's driver set-up (surfdisp96.f:124-217): 0.9 x 0.95 x the Rayleigh velocity of the slowest layer, binary32"""
    betmn, jmn, jsol = f32(1.0e20), 0, 1
    for i in range(b.size):
        bi, ai = f32(b[i]), f32(a[i])
        if bi > f32(0.01) and bi < betmn:
            betmn, jmn, jsol = bi, i, 1
        elif bi <= f32(0.01) and ai < betmn:
            betmn, jmn, jsol = ai, i, 0
    c = betmn if jsol == 0 else f32(O.gtsolh(a[jmn], b[jmn]))
    return float(f32(0.90) * (f32(0.95) * c))


def skip_rule(d, b, rho, cm, omega, J):
    """(m, b_m, value bound, q condition, value condition) for one model: d, b, rho its layers (binary32 values as float64)"""
    n = b.size
    if n < 2:
        return 0, cm, 0.0, False, False
    vmin = float(b.min())
    mumin = float((rho * (b * b)).min())
    dmax = float(d[:n - 1].max())
    lim = vmin - DC
    ok_q = dmax * omega <= 4.5e4 * cm
    ok_v = (mumin * mumin) * ((omega * omega) * DC) >= 1.0e-18 * (vmin * vmin * vmin)
    bound = mumin * omega * np.sqrt(DC / vmin ** 3) if vmin > 0 else 0.0
    m, bm = 0, cm
    if omega > 0.0 and ok_q and ok_v:
        while True:
            bn = (J - 1 if m == 0 else J) * DC + bm
            if not (2.0 * DC + bn <= lim):
                break
            bm, m = bn, m + 1
    return m, bm, bound, ok_q, ok_v


def skipped_points(cm, m, J):
    """the grid points of the scan's first m rounds, then the two leading trials of round m + 1 (m >= 1)"""
    pts, b = [cm] + [r * DC + cm for r in range(1, J)], (J - 1) * DC + cm
    for _ in range(m - 1):
        pts += [(r + 1) * DC + b for r in range(J)]
        b = J * DC + b
    return np.array(pts), np.array([1.0 * DC + b, 2.0 * DC + b]), b


def columns(models, i):
    nlay, h, vp, vs, rho = models
    n = int(nlay[i])
    return [np.ascontiguousarray(x[:n, i], dtype=f32) for x in (h, vp, vs, rho)]


def rule_of(O, models, i, omega, J):
    d, a, b, rho = columns(models, i)
    cm = start_value(O, a, b)
    return (cm,) + skip_rule(d.astype(float), b.astype(float), rho.astype(float), cm, omega, J)


# ---- the model families ----------------------------------------------------------------------------------------------------------
def with_vmin_at(models, where):
    """the slowest layer moved to the top, the middle or the half-space: 0.8 x the model's slowest, vp and rho with it"""
    nlay, h, vp, vs, rho = [x.copy() for x in models]
    for i in range(nlay.size):
        n = int(nlay[i])
        p = {"top": 0, "middle": n // 2, "halfspace": n - 1}[where]
        k = vp[p, i] / vs[p, i]
        vs[p, i] = 0.8 * vs[:n, i].min()
        vp[p, i] = k * vs[p, i]
        rho[p, i] = 0.32 * vp[p, i] + 0.77
    return nlay, h, vp, vs, rho


def family(name):
    """(models, first period of every model)"""
    rs = np.random.RandomState(abs(hash_of(name)))
    if name == "bench":
        return synth_models(np.random.RandomState(SEED), N, 10, lvz_frac=0.1), np.full(N, SWD_PERIODS[0])
    if name == "prior":
        return prior_models(rs, N, 21), rs.uniform(1.0, 60.0, N)
    if name == "lvz":
        return synth_models(rs, N, 12, lvz_frac=0.25, ragged=True), rs.uniform(1.0, 60.0, N)
    base = prior_models(rs, N, 12, nmin=3)
    return with_vmin_at(base, name[5:]), rs.uniform(1.0, 60.0, N)


def hash_of(name):
    return 1000 + sum(ord(c) * (i + 1) for i, c in enumerate(name))


FAMILIES = ("bench", "prior", "lvz", "vmin_top", "vmin_middle", "vmin_halfspace")
_cache = {}


def cached_family(name):
    if name not in _cache:
        _cache[name] = family(name)
    return _cache[name]


# ---- the tests -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", LANES)
@pytest.mark.parametrize("name", FAMILIES)
def test_no_skipped_point_could_have_held_a_sign_change_or_fired_the_guard(oracle, name, J):
    models, periods = cached_family(name)
    lib = oracle.lib()
    lib.bho_dltar1.restype = C.c_double
    fp = C.POINTER(C.c_float)
    ms, worst, worst_ratio, npts = [], np.inf, np.inf, 0
    for i in range(N):
        d, a, b, rho = columns(models, i)
        omega = 2.0 * np.pi / periods[i]
        cm = start_value(oracle, a, b)
        m, bm, bound, ok_q, ok_v = skip_rule(d.astype(float), b.astype(float), rho.astype(float), cm, omega, J)
        ms.append(m)
        if m == 0:
            continue
        pts, lead, b_end = skipped_points(cm, m, J)
        assert b_end == bm                                                   # the kernel's start value is the scan's own grid point
        vmin = float(b.min())
        assert pts.max() <= bm < lead[0] < lead[1] <= vmin - DC
        assert 2.0 * DC + (J * DC + bm) > vmin - DC                                    # m is the largest such count
        pd_, pb_, pr_ = d.ctypes.data_as(fp), b.ctypes.data_as(fp), rho.ctypes.data_as(fp)
        llw = 1
        for c in np.concatenate((pts, lead)):
            f = lib.bho_dltar1(C.c_double(omega / c), C.c_double(omega), pd_, pb_, pr_, int(b.size), llw)
            worst = min(worst, f)
            worst_ratio = min(worst_ratio, f / min(1.0, bound))
            npts += 1
    ms = np.array(ms)
    print("%s, %d lanes: rounds skipped mean %.2f min %d max %d; %d points, smallest value %.3e, smallest value / bound %.3f"
          % (name, J, ms.mean(), ms.min(), ms.max(), npts, worst, worst_ratio))
    assert (ms > 0).mean() > 0.9                                             # (the family does exercise the rule)
    assert worst >= MARGIN * FLOOR                                           # positive, and the stated margin above the floor
    assert worst_ratio >= 1.0 - 1.0e-9                                       # the derived lower bound is one


def one_model(vs, h, rho=None, vpvs=1.75):
    vs, h = np.array(vs, dtype=float), np.array(h, dtype=float)
    vp = vpvs * vs
    rho = 0.32 * vp + 0.77 if rho is None else np.array(rho, dtype=float)
    return np.array([vs.size], dtype=np.int32), h[:, None], vp[:, None], vs[:, None], rho[:, None]


M0_CASES = {
    # a soft top layer: cm = 0.79 vmin is then within three steps of vmin
    "start value within three steps of vmin": one_model([0.06, 2.5, 3.5], [0.5, 10.0, 0.0]),
    # q = d rb can pass 9e4: dmax omega > 4.5e4 cm
    "a layer thick enough to break the q bound": one_model([2.8, 3.4, 4.2], [5.0, 1.0e5, 0.0]),
    # rho -> mu rb below 1e-9
    "a density small enough to break the value bound": one_model([2.8, 3.4, 4.2], [5.0, 12.0, 0.0], rho=[2.6, 1.0e-9, 3.1]),
}


@pytest.mark.parametrize("case", sorted(M0_CASES))
def test_the_rule_gives_no_skip(oracle, case):
    models = M0_CASES[case]
    omega = 2.0 * np.pi / SWD_PERIODS[0]
    healthy = one_model([2.8, 3.4, 4.2], [5.0, 12.0, 0.0])
    for J in (4, 8, 16, 32, 64):
        cm, m, bm, bound, ok_q, ok_v = rule_of(oracle, models, 0, omega, J)
        assert m == 0 and bm == cm, (J, m)
        assert rule_of(oracle, healthy, 0, omega, J)[1] > 0
        if "three steps" in case:
            assert ok_q and ok_v and cm + 3.0 * DC > float(models[3][:, 0].min()) - DC
        elif "thick" in case:
            assert not ok_q and ok_v
        else:
            assert ok_q and not ok_v


def test_rounds_skipped_on_the_bench_models(oracle):
    """1024 of bench.py's models (its seed), 16 lanes, its first period: 5.40 rounds per model, at least 4, at most 8 -- and the
    schedule model's optional argument (tools/cpu_lean_schedule.py) applies the same rule"""
    models = synth_models(np.random.RandomState(20260927), 1024, 10, lvz_frac=0.1)
    omega = 2.0 * np.pi / SWD_PERIODS[0]
    m = np.array([rule_of(oracle, models, i, omega, 16)[1] for i in range(1024)])
    print("rounds skipped: mean %.4f min %d max %d" % (m.mean(), m.min(), m.max()))
    assert abs(m.mean() - 5.40) < 0.005 and m.min() == 4 and m.max() == 8
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import cpu_lean_schedule as S
    assert np.array_equal(S.love_skip_rounds(*models, SWD_PERIODS, 16), m)
