"""The dispersion kernels' fast arithmetic (csrc/swd_fa.h, csrc/swd_lean.hip) value by value: the functions of namespace fa
(bh_probe_math ops 17-23) against mpmath at the epsilons of tests/swd_fa_ref.py, and the three secular evaluators
(bh_probe_swd_secular: 0 exact, 1 fa::*_secular, 2 lean_*) at the same points -- the exact one to the bits of the reference's
binary64 arithmetic (oracle.dltar), the fast ones within FACTOR x fa_bound of the long-double value.  The bound is proven on the
CPU first (tests/test_swd_fa_ref.py); nothing here is fitted to what the device returns.  Every launch is a few thousand lanes."""
import mpmath
import numpy as np
import pytest

import swd_fa_ref as R
from bayhunter_amd import engine as E
from oracle import oracle as O

pytestmark = pytest.mark.gpu
LD = np.longdouble
OP_RCP, OP_RCP1, OP_SQRT, OP_RSQRT, OP_SIN, OP_COS, OP_EXPNEG = 17, 18, 19, 20, 21, 22, 23
NAMES = {1: "Love", 2: "Rayleigh"}


def _mp_err(got, x, f, relative):
    """max over the inputs of |got - f(x)| (divided by |f(x)| if relative), the difference taken in mpmath"""
    worst = 0.0
    with mpmath.workdps(45):
        for g, v in zip(got, x):
            want = f(mpmath.mpf(float(v)))
            err = abs(mpmath.mpf(float(g)) - want)
            worst = max(worst, float(err / abs(want)) if relative else float(err))
    return worst


# ---- the functions of namespace fa ------------------------------------------------------------------------------------------------
def test_rcp_and_rcp1(engine):
    rs = np.random.RandomState(11)
    mag = 10.0 ** rs.uniform(-30, 30, 3000)
    vel = rs.uniform(0.01, 100.0, 600).astype(np.float32).astype(np.float64)           # binary32-valued velocities
    rho = np.concatenate([rs.uniform(0.001, 10.0, 300), 10.0 ** rs.uniform(0, 6, 300), [999999.0, 0.001]]).astype(np.float32).astype(np.float64)
    omega = 2 * np.pi / rs.uniform(0.5, 100.0, 600)
    diff = 10.0 ** rs.uniform(-12, 0, 600) * rs.choice([-1.0, 1.0], 600)               # fhi - flo of a closing bracket
    pow2 = 2.0 ** np.arange(-100, 101)
    x = np.concatenate([mag, -mag[:1000], vel, rho, omega, diff, pow2, -pow2])
    assert np.all(np.isfinite(engine.probe_math(OP_RCP, x)))
    for op, name in ((OP_RCP, "rcp"), (OP_RCP1, "rcp1")):
        got = engine.probe_math(op, x)
        worst = _mp_err(got, x, lambda v: 1 / v, True)
        print("fa::%s: relative error %.4g u (eps %.4g u) on %d inputs" % (name, worst / R.U, R.EPS_FA[name] / R.U, x.size))
        assert worst <= R.EPS_FA[name], (name, worst)
    assert np.array_equal(engine.probe_math(OP_RCP, pow2), 1.0 / pow2)                  # powers of two: exact


def test_sqrt_rsqrt(engine):
    rs = np.random.RandomState(12)
    near = np.concatenate([m * (1 + s * np.arange(0, 6) * 2.0 ** -52) for m in (1.0, 2.0, 4.0) for s in (1, -0.5)])
    near = np.concatenate([near * 2.0 ** e for e in (-960, -101, -2, -1, 0, 1, 2, 17, 18)])
    x = np.concatenate([10.0 ** rs.uniform(-290, 6, 4000), rs.uniform(1e-6, 1e6, 1000), near, [1.0e-290, 1.0e6, 1.0]])
    xl = x.astype(LD)
    for op, name, want in ((OP_SQRT, "sqrt", np.sqrt(xl)), (OP_RSQRT, "rsqrt", 1 / np.sqrt(xl))):
        got = engine.probe_math(op, x)
        rel = float(np.max(np.abs((got.astype(LD) - want) / want)))                   # (long double: 2^-11 u of its own)
        print("fa::sqrt_rsqrt %s: relative error %.4g u (eps %.4g u) on %d inputs" % (name, rel / R.U, R.EPS_FA[name] / R.U, x.size))
        assert rel <= R.EPS_FA[name], (name, rel)


def test_sincos(engine):
    rs = np.random.RandomState(13)
    n = np.unique(np.concatenate([np.arange(1, 200), rs.randint(1, 57001, 400), [57000, 56999, 57295, 57296]])).astype(np.float64)
    at = n * (np.pi / 2)
    ulp = np.spacing(at)
    x = np.concatenate([rs.uniform(0, 10, 2000), rs.uniform(0, 9.0e4, 3000)] + [at + j * ulp for j in (-2, -1, 0, 1, 2)] + [[9.0e4, 0.0]])
    x = x[x <= 9.0e4]
    small = x < np.pi / 4
    for op, name, f in ((OP_SIN, "sin", mpmath.sin), (OP_COS, "cos", mpmath.cos)):
        got = engine.probe_math(op, x)
        worst = _mp_err(got, x, f, False)
        print("fa::sincos %s: absolute error %.4g u (eps %.4g u) on %d inputs" % (name, worst / R.U, R.EPS_FA["sin"] / R.U, x.size))
        assert worst <= R.EPS_FA["sin"], (name, worst)
    xs = x[small & (x > 0)]
    rel = _mp_err(engine.probe_math(OP_SIN, xs) / xs, xs, lambda v: mpmath.sin(v) / v, False)
    print("fa::sincos sin below pi/4: error / x %.4g u (sin_small %.4g u)" % (rel / R.U, R.EPS_FA["sin_small"] / R.U))
    assert rel <= R.EPS_FA["sin_small"] + R.U                                           # (+ u: the division by x above)
    z = engine.probe_math(OP_SIN, np.zeros(1)), engine.probe_math(OP_COS, np.zeros(1))
    assert z[0][0] == 0.0 and z[1][0] == 1.0


def test_expneg(engine):
    rs = np.random.RandomState(14)
    kl = np.arange(0, 1010) * np.log(2.0)
    x = np.concatenate([rs.uniform(0, 3, 1000), rs.uniform(0, 700, 3000), kl, kl + np.spacing(kl), np.maximum(kl - np.spacing(kl), 0.0), [0.0, 700.0]])
    x = x[x <= 700.0]
    got = engine.probe_math(OP_EXPNEG, x)
    assert np.all(got >= 2.2250738585072014e-308), "a normal result is required up to 700"
    worst = _mp_err(got, x, lambda v: mpmath.exp(-v), True)
    print("fa::expneg: relative error %.4g u (eps %.4g u) on %d inputs" % (worst / R.U, R.EPS_FA["exp"] / R.U, x.size))
    assert worst <= R.EPS_FA["exp"], worst
    assert got[-2] == 1.0


# ---- the three evaluators -----------------------------------------------------------------------------------------------------
def _filler(mdl, extra=3):
    """the model's rows followed by `extra` NaN rows (the ragged filler of a batch)"""
    return [np.concatenate([x, np.full(extra, np.nan, dtype=np.float32)]) for x in mdl]


def _probe_all(engine, ifunc, mdl, k, om):
    """{evaluator: values} at mtop = mmax; asserts that mtop = mmax + 3 with NaN filler gives the same bits (evaluator 2 has rows
    for 32 layers: with 32 layers of its own there is no room for filler, and the call is refused)"""
    mmax = mdl[0].size
    out = {}
    for ev in (0, 1, 2):
        out[ev] = engine.probe_swd_secular(ev, ifunc, mmax, mdl[0], mdl[1], mdl[2], mdl[3], k, om)
        if ev == 2 and mmax + 3 > 32:
            continue
        rag = engine.probe_swd_secular(ev, ifunc, mmax, *_filler(mdl), k, om)
        assert np.array_equal(rag.view(np.int64), out[ev].view(np.int64)), "evaluator %d reads the ragged filler" % ev
    return out


def _oracle(ifunc, mdl, k, om):
    return np.array([O.dltar(float(k[i]), float(om[i]), ifunc, *mdl) for i in range(k.size)])


def _same_bits(a, b):
    return np.array_equal(a.view(np.int64)[~(np.isnan(a) & np.isnan(b))], b.view(np.int64)[~(np.isnan(a) & np.isnan(b))])


def _poison(ref):
    """(must be NaN, must be a number): r d of some layer above 9e4 by more than its bound / of every layer below by more"""
    with np.errstate(invalid="ignore"):
        return np.any(ref.q - ref.q_bound > R.POISON, axis=0), np.all(ref.q + ref.q_bound < R.POISON, axis=0)


def _check_fast(name, ifunc, ev, got, ref):
    """evaluator `ev` against the reference; returns the error / bound ratios of the asserted points"""
    must_nan, must_num = _poison(ref)
    assert not np.any(np.isinf(got)), (name, ifunc, ev)
    assert np.all(np.isnan(got[must_nan])), (name, ifunc, ev, "poisoned points must be NaN")
    assert not np.any(np.isnan(got[must_num])), (name, ifunc, ev, np.flatnonzero(np.isnan(got) & must_num))
    err = np.abs(got[must_num].astype(LD) - ref.value[must_num]).astype(np.float64)
    bnd = ref.fa_bound[must_num]
    bad = np.flatnonzero(~(err <= R.FACTOR * bnd))
    assert bad.size == 0, (name, NAMES[ifunc], "evaluator %d" % ev, np.flatnonzero(must_num)[bad], err[bad], bnd[bad])
    return err / bnd


@pytest.fixture(scope="module")
def pop():
    return [(name, ifunc, mdl, k, om, kind, dist, R.secular_ref(ifunc, mdl[0], mdl[1], mdl[2], mdl[3], k, om))
            for name, ifunc, mdl, k, om, kind, dist in R.population()]


def test_evaluators_on_the_population(engine, pop):
    """Layer counts 2, 3, 4, 5, 12, 32; sorted-velocity, LVZ and bound-corner models; 64 points each (uniform, near a layer
    velocity, near a half-space velocity); with and without ragged filler."""
    ratios = {(i, ev): [] for i in (1, 2) for ev in (1, 2)}
    diffs = {(i, ev): [] for i in (1, 2) for ev in (1, 2)}
    for name, ifunc, mdl, k, om, kind, dist, ref in pop:
        got = _probe_all(engine, ifunc, mdl, k, om)
        assert _same_bits(got[0], _oracle(ifunc, mdl, k, om)), (name, NAMES[ifunc], "the device's exact arithmetic is not the reference's bits")
        for ev in (1, 2):
            ratios[ifunc, ev].append(_check_fast(name, ifunc, ev, got[ev], ref))
            ok = np.isfinite(got[ev]) & np.isfinite(got[0])
            diffs[ifunc, ev].append(np.abs(got[ev][ok] - got[0][ok]))
    for (ifunc, ev), r in sorted(ratios.items()):
        r, dd = np.concatenate(r), np.concatenate(diffs[ifunc, ev])
        dec = np.floor(np.log10(np.maximum(dd, 1e-18))).astype(int)
        hist = ", ".join("1e%d: %d" % (e, int(np.sum(dec == e))) for e in range(-18, 1) if np.any(dec == e))
        print("%s, evaluator %d: worst error / fa_bound %.3g over %d points; |f_fast - f_exact(device)| max %.3g, below 1e-11 in %.1f %%; by decade {%s}"
              % (NAMES[ifunc], ev, r.max(), r.size, dd.max(), 100 * np.mean(dd < 1e-11), hist))


@pytest.mark.parametrize("ifunc", [1, 2])
def test_exact_limit_branch(engine, ifunc):
    """wvno = omega * fa::rcp(v_m), one IEEE multiply as the kernels form omega * rcp(b): k == xk holds exactly for layer m and the
    `zero` branch of wave() / love_terms() (or the half-space's r = 0) runs.  A finite layer and the half-space."""
    rs = np.random.RandomState(15 + ifunc)
    mdl = R.lvz_model(rs, 5)
    om = 2 * np.pi / rs.uniform(0.5, 100.0, 32)
    for m in (2, 4):
        for v in ([mdl[2][m]] if ifunc == 1 else [mdl[2][m], mdl[1][m]]):
            r = engine.probe_math(OP_RCP, np.array([float(v)]))[0]
            k = om * r
            ref = R.secular_ref(ifunc, mdl[0], mdl[1], mdl[2], mdl[3], k, om)
            got = _probe_all(engine, ifunc, mdl, k, om)
            assert _same_bits(got[0], _oracle(ifunc, mdl, k, om))
            for ev in (1, 2):
                rr = _check_fast("limit layer %d" % m, ifunc, ev, got[ev], ref)
                print("%s, evaluator %d, k == omega rcp(%g) (layer %d): worst error / fa_bound %.3g" % (NAMES[ifunc], ev, v, m, rr.max()))


@pytest.mark.parametrize("ifunc", [1, 2])
def test_poison_rule(engine, ifunc):
    """One layer thick enough that r d passes 9e4 at short periods: NaN exactly where the long-double r d of some layer lies above
    9e4 by more than its bound, numbers (within the bound) where every layer's lies below by more than its bound."""
    rs = np.random.RandomState(17 + ifunc)
    d = np.array([2.0, 2.0e6, 5.0, 0.0], dtype=np.float32)
    vs = np.array([3.0, 3.5, 3.9, 4.5], dtype=np.float32)
    vp = (1.75 * vs).astype(np.float32)
    rho = (0.77 + 0.32 * vp).astype(np.float32)
    mdl = (d, vp, vs, rho)
    k, om, kind, dist = R.points(rs, ifunc, d, vp, vs, n=128)
    ref = R.secular_ref(ifunc, d, vp, vs, rho, k, om)
    must_nan, must_num = _poison(ref)
    assert must_nan.sum() >= 10 and must_num.sum() >= 10, (must_nan.sum(), must_num.sum())
    got = _probe_all(engine, ifunc, mdl, k, om)
    assert np.all(np.isfinite(got[0])) and _same_bits(got[0], _oracle(ifunc, mdl, k, om))
    for ev in (1, 2):
        rr = _check_fast("thick", ifunc, ev, got[ev], ref)
        print("%s, evaluator %d: %d poisoned, %d numbers (worst error / fa_bound %.3g), %d not asserted"
              % (NAMES[ifunc], ev, must_nan.sum(), must_num.sum(), rr.max(), (~must_nan & ~must_num).sum()))


def test_bound_corner_model(engine, pop):
    """SearchT::init's sanity bounds at their corners: a finite value within the bound or the expected NaN, never inf -- the lean
    evaluator's "two layers cannot leave the binary64 range"."""
    for name, ifunc, mdl, k, om, kind, dist, ref in pop:
        if name != "corner":
            continue
        got = _probe_all(engine, ifunc, mdl, k, om)
        must_nan, must_num = _poison(ref)
        for ev in (0, 1, 2):
            assert not np.any(np.isinf(got[ev])), (NAMES[ifunc], ev)
        assert np.all(np.isfinite(got[0]))
        for ev in (1, 2):
            rr = _check_fast(name, ifunc, ev, got[ev], ref)
            print("%s corner model, evaluator %d: %d NaN as expected, %d numbers, worst error / fa_bound %.3g"
                  % (NAMES[ifunc], ev, must_nan.sum(), must_num.sum(), rr.max() if rr.size else 0.0))


def test_probe_refusals_leave_out_untouched(engine):
    rs = np.random.RandomState(19)
    mdl = R.sorted_model(rs, 4)
    k, om = np.full(8, 1.0), np.full(8, 3.0)

    def refused(ev, ifunc, mmax, rows):
        out = np.full(8, 7.0)
        m = [np.resize(x, rows) for x in mdl]
        with pytest.raises(E.EngineError):
            engine.probe_swd_secular(ev, ifunc, mmax, m[0], m[1], m[2], m[3], k, om, out=out)
        assert np.all(out == 7.0)

    refused(3, 1, 4, 4)          # no such evaluator
    refused(-1, 2, 4, 4)
    refused(0, 3, 4, 4)          # no such wave type
    refused(1, 0, 4, 4)
    refused(0, 1, 1, 4)          # a half-space alone
    refused(1, 2, 5, 4)          # more layers than rows
    refused(2, 2, 4, 33)         # the lean kernel's arrays end at 32 rows
    refused(0, 2, 4, 101)        # the Fortran's limit
    refused(1, 1, 4, 101)
    out = engine.probe_swd_secular(2, 2, 4, *[np.resize(x, 32) for x in mdl], k, om)     # 32 and 100 rows are served
    assert np.all(np.isfinite(out))
    assert np.all(np.isfinite(engine.probe_swd_secular(0, 1, 4, *[np.resize(x, 100) for x in mdl], k, om)))
