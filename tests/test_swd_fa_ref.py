"""The reference of the dispersion fast-arithmetic tests (tests/swd_fa_ref.py) checked on the CPU: its long-double value against
mpmath, its error analysis against the reference's own binary64 arithmetic (oracle.dltar), and that its bound says something.
What makes the GPU tests of tests/test_gpu_swd_fa.py safe to trust: the bound they assert is proven here first."""
import mpmath
import numpy as np
import pytest

import swd_fa_ref as R
from oracle import oracle

LD = np.longdouble


@pytest.fixture(scope="module")
def pop():
    """the population with its reference, computed once"""
    return [(name, ifunc, mdl, k, om, kind, dist, R.secular_ref(ifunc, mdl[0], mdl[1], mdl[2], mdl[3], k, om))
            for name, ifunc, mdl, k, om, kind, dist in R.population()]


def _ld_to_mp(x):
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - LD(hi)))


def secular_mp(ifunc, d, a, b, rho, k, om):
    """The same function from the formulas in mpmath (scalar; unscaled cosh / sinh -- mpmath has the range), for one point"""
    mp = mpmath.mpf
    d, a, b, rho = [[mp(float(v)) for v in x] for x in (d, a, b, rho)]
    k, om = mp(float(k)), mp(float(om))
    n = len(d)

    def terms(xk, dm):
        r2 = (k + xk) * abs(k - xk)
        r = mpmath.sqrt(r2)
        q = r * dm
        if r2 == 0:
            return mp(1), dm, mp(0)
        if k < xk:
            return mpmath.cos(q), mpmath.sin(q) / r, -r * mpmath.sin(q)
        return mpmath.cosh(q), mpmath.sinh(q) / r, r * mpmath.sinh(q)

    if ifunc == 1:
        xkb = om / b[-1]
        e1, e2 = rho[-1] * mpmath.sqrt((k + xkb) * abs(k - xkb)), 1 / (b[-1] * b[-1])
        for m in range(n - 2, -1, -1):
            xmu = rho[m] * b[m] * b[m]
            c, y, z = terms(om / b[m], d[m])
            e1, e2 = e1 * c + e2 * xmu * z, e1 * y / xmu + e2 * c
        return e1 / max(abs(e1), abs(e2))
    k2 = k * k
    xka, xkb = om / a[-1], om / b[-1]
    ra, rb = mpmath.sqrt((k + xka) * abs(k - xka)), mpmath.sqrt((k + xkb) * abs(k - xkb))
    gammk = 2 * (b[-1] / om) ** 2
    gam = gammk * k2
    g1 = gam - 1
    r1 = rho[-1]
    e = [r1 * r1 * (g1 * g1 - gam * gammk * ra * rb), -r1 * ra, r1 * (g1 - gammk * ra * rb), r1 * rb, k2 - ra * rb]
    for m in range(n - 2, -1, -1):
        gammk = 2 * (b[m] / om) ** 2
        gam = gammk * k2
        cosp, w, x = terms(om / a[m], d[m])
        cosq, y, z = terms(om / b[m], d[m])
        a0 = mp(1)                                              # var's a0 without its scaling: the unscaled matrix has a0 = 1
        rh = rho[m]
        g1 = gam - 1
        tw = gam + g1
        gg, gs = gam * gammk, g1 * g1
        cpcq, cpy, cpz, cqw, cqx = cosp * cosq, cosp * y, cosp * z, cosq * w, cosq * x
        xy, xz, wy, wz = x * y, x * z, w * y, w * z
        a0pq = a0 - cpcq
        ca11 = cpcq - 2 * gam * g1 * a0pq - gg * xz - k2 * gs * wy
        ca12 = (k2 * cpy - cqx) / rh
        ca13 = -(tw * a0pq + gammk * xz + k2 * g1 * wy) / rh
        ca14 = (cpz - k2 * cqw) / rh
        ca15 = -(2 * k2 * a0pq + xz + k2 * k2 * wy) / (rh * rh)
        ca21 = (gg * cpz - gs * cqw) * rh
        ca22 = cpcq
        ca23 = gammk * cpz - g1 * cqw
        ca24 = -wz
        ca41 = (gs * cpy - gg * cqx) * rh
        ca42 = -xy
        ca43 = g1 * cpy - gammk * cqx
        ca51 = -(2 * gg * gs * a0pq + gg * gg * xz + gs * gs * wy) * rh * rh
        ca53 = -(gammk * g1 * tw * a0pq + gam * gammk * gammk * xz + g1 * gs * wy) * rh
        t = -2 * k2
        ca31, ca32, ca34, ca35 = t * ca53, t * ca43, t * ca23, t * ca13
        ca33 = a0 + 2 * (cpcq - ca11)
        ca = [[ca11, ca12, ca13, ca14, ca15], [ca21, ca22, ca23, ca24, ca14], [ca31, ca32, ca33, ca34, ca35],
              [ca41, ca42, ca43, ca22, ca12], [ca51, ca41, ca53, ca21, ca11]]
        e = [sum(e[j] * ca[j][i] for j in range(5)) for i in range(5)]
    return e[0] / max(abs(v) for v in e)


def test_long_double_value_against_mpmath(pop):
    """|LD - mp| <= FACTOR x ref_bound at 60 digits (the corner model's 6e6 radians cost 7 of them): 8 points of every model --
    4 uniform, 2 near a layer velocity, 2 near a half-space velocity -- and all 64 of each bound-corner model."""
    n, worst, skipped = 0, 0.0, 0
    with mpmath.workdps(60):
        for name, ifunc, mdl, k, om, kind, dist, ref in pop:
            sel = range(k.size) if name == "corner" else np.concatenate([np.flatnonzero(kind == 0)[:4], np.flatnonzero(kind == 1)[:2],
                                                                         np.flatnonzero(kind == 2)[:2]])
            for i in sel:
                if not np.isfinite(ref.ref_bound[i]):
                    skipped += 1
                    continue
                want = secular_mp(ifunc, mdl[0], mdl[1], mdl[2], mdl[3], k[i], om[i])
                err = float(abs(_ld_to_mp(ref.value[i]) - want))
                assert err <= R.FACTOR * ref.ref_bound[i], (name, ifunc, i, err, ref.ref_bound[i])
                worst = max(worst, err / ref.ref_bound[i])
                n += 1
    print("long double against mpmath: %d points, worst error / ref_bound %.3g, %d with an infinite bound skipped" % (n, worst, skipped))
    assert n >= 200 and skipped == 0


def test_reference_arithmetic_obeys_the_analysis(pop):
    """oracle.dltar -- the reference's dltar1 / dltar4 in binary64 -- within FACTOR x f64_bound of the long-double value, every point"""
    worst = 0.0
    for name, ifunc, mdl, k, om, kind, dist, ref in pop:
        got = np.array([oracle.dltar(float(k[i]), float(om[i]), ifunc, *mdl) for i in range(k.size)])
        assert np.all(np.isfinite(got)), name
        err = np.abs(got.astype(LD) - ref.value).astype(np.float64)
        bad = np.flatnonzero(~(err <= R.FACTOR * ref.f64_bound))
        assert bad.size == 0, (name, ifunc, bad, err[bad], ref.f64_bound[bad])
        worst = max(worst, float(np.max(err / ref.f64_bound)))
    print("binary64 reference arithmetic: worst error / f64_bound %.3g (FACTOR %g)" % (worst, R.FACTOR))


def test_bound_is_not_vacuous(pop):
    """At most 10 % of the uniformly drawn points have FACTOR x fa_bound above 1e-9; f64_bound <= fa_bound everywhere; the
    near-velocity points counted by decade of their distance."""
    uni, near = [], {1: [], 2: []}
    for name, ifunc, mdl, k, om, kind, dist, ref in pop:
        assert np.all(ref.f64_bound <= ref.fa_bound), name
        assert np.all(ref.ref_bound <= 2.0 ** -9 * ref.f64_bound + 1e-300), name
        uni.append(R.FACTOR * ref.fa_bound[kind == 0])
        for kd in (1, 2):
            s = kind == kd
            near[kd] += list(zip(np.floor(np.log10(dist[s])).astype(int), R.FACTOR * ref.fa_bound[s]))
    uni = np.concatenate(uni)
    frac = float(np.mean(~(uni <= 1e-9)))
    print("uniform points: %d, FACTOR x fa_bound above 1e-9 in %.1f %%, median %.2e" % (uni.size, 100 * frac, np.median(uni)))
    for kd, what in ((1, "a layer velocity"), (2, "a half-space velocity")):
        for dec in range(-12, -6):
            b = np.array([v for d_, v in near[kd] if d_ == dec])
            if b.size:
                print("within 1e%d of %s: %d points, %d with FACTOR x fa_bound above 1e-9, median %.2e" % (dec + 1, what, b.size, int(np.sum(~(b <= 1e-9))), np.median(b)))
    assert frac <= 0.10


def test_epsilons_are_a_few_ulp():
    """swd_fa.h: "within a few units in the last place": the four derived epsilons stay below 8 u, and no smaller than IEEE's"""
    for name in ("rcp", "sqrt", "rsqrt", "sin", "exp"):
        assert R.U <= R.EPS_FA[name] <= 8 * R.U, name
    assert R.EPS_FA["rcp1"] <= 2.0 ** -45
    for name in R.EPS_FA:
        assert R.EPS_F64[name] <= R.EPS_FA[name]
