"""The Rayleigh ellipticity's restatement (tests/ellip_ref.py: include/bh_engine_swd_ellip.h in plain Python) against what does not
share its formulas: the motion-stress ODE of Aki & Richards carried through the layers in longdouble, the closed form of a
half-space, the sign of the particle motion over a slow sediment -- and the polish against the root bisected to the last bit; the
gate on the mismatch and where its constant comes from.  No GPU.  `python tests/test_ellip_ref.py` writes the worst values into profiles/swd_ellip_accuracy.txt.

Where the bounds come from.  The restatement's rounding error at the root is a few 1e-15 over these stacks (its own two ratios
differ by <= 1.2e-14 there) and the ODE route's, in longdouble, less; 1e-9 for the ODE's self-consistency keeps the comparison
away from where Thomson-Haskell propagation breaks down (it drifts by per cents there), 1e-10 for the restatement against it is
five orders below the O(1) error of a wrong component, a missing k or a sign slip; 1e-12 for the closed form and for the polish
is |d ln hv / d ln c| <= 100 times the 1e-16 to which a float64 root is known, with a decade to spare."""
import math
import os

import numpy as np
import pytest

import ellip_ref as R
from conftest import REPO

ROOTS = {name: R.fundamental_roots(m, R.PERIODS) for name, m in R.MODELS.items()}


def rel(a, b):
    return abs(float((np.longdouble(a) - np.longdouble(b)) / np.longdouble(b)))


def ode_table():
    """every (model, period): (hv of the restatement at the bisected root, the ODE's two ratios there)"""
    out = {}
    for name, m in R.MODELS.items():
        for T, c in zip(R.PERIODS, ROOTS[name]):
            out[name, T] = (R.ellip(m, T, c, 0)[0],) + R.ode_ratios(m, T, c)
    return out


ODE = ode_table()


def test_ode_route_is_self_consistent_on_every_pair():
    worst = max(rel(o1, o2) for _, o1, o2 in ODE.values())
    print("ODE self-consistency, worst of %d pairs: %.2e" % (len(ODE), worst))
    assert len(ODE) == 24
    for key, (_, o1, o2) in ODE.items():
        assert rel(o1, o2) <= 1e-9, key


def test_restatement_agrees_with_the_ode_route():
    worst = max(rel(abs(hv), abs(o1)) for hv, o1, _ in ODE.values())
    print("restatement against ODE, worst: %.2e" % worst)
    for key, (hv, o1, o2) in ODE.items():
        assert rel(abs(hv), abs(o1)) <= 1e-10, key
        assert rel(abs(hv), abs(o2)) <= 1e-10, key
        assert (hv > 0) == (o1 < 0) == (o2 < 0), key   # the ODE's convention is the opposite one


def test_sign_pattern_of_the_sediment_model():
    """retrograde (positive) at short periods, prograde between ~1.8 and ~3.5 s, retrograde with a peak at 4 s and beyond"""
    m = R.MODELS["sediment"]
    Ts = [1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 8.0, 20.0]
    hv = [R.ellip(m, T, c)[0] for T, c in zip(Ts, R.fundamental_roots(m, Ts))]
    assert [v > 0 for v in hv] == [True, True, False, False, False, True, True, True]
    assert hv[2] == pytest.approx(-0.957, abs(2e-3)) and hv[5] == pytest.approx(3.565, abs(2e-3))
    assert all(v > 0 for name in ("poisson", "crust", "lvz") for v, _, _ in [ODE[name, T] for T in R.PERIODS])


def closed_form_worst():
    m = R.MODELS["poisson"]
    cf = R.halfspace_hv(m[1][0], m[2][0])
    x = R.halfspace_x(m[1][0], m[2][0])
    c_cf = float(np.longdouble(m[2][0]) * np.sqrt(x))
    return max(rel(R.ellip(m, T, c, 0)[0], cf) for T, c in zip(R.PERIODS, ROOTS["poisson"])), \
        max(abs(c - c_cf) / c_cf for c in ROOTS["poisson"]), float(cf)


def test_homogeneous_stack_against_the_closed_form():
    worst, worst_c, cf = closed_form_worst()
    print("closed form %.14f, worst relative difference %.2e (root: %.2e)" % (cf, worst, worst_c))
    assert cf == pytest.approx(0.68125004878, abs=1e-10)   # Poisson solid: 2 sqrt(1 - x) / (2 - x) at x = 2 - 2 / sqrt(3), binary32 velocities
    assert worst <= 1e-12
    assert worst_c <= 1e-14


def polish_table():
    """every (model, period, side): hv at the root, then per nsteps (error of hv, mismatch, flag) from c (1 +- 2e-6)"""
    out = {}
    for name, m in R.MODELS.items():
        for T, c in zip(R.PERIODS, ROOTS[name]):
            hv0 = R.ellip(m, T, c, 0)[0]
            for side in (-1.0, 1.0):
                rows = []
                for nsteps in (0, 1, 2, 3):
                    hv, mis, cpol, flag = R.ellip(m, T, c * (1.0 + side * 2.0e-6), nsteps)
                    rows.append((rel(hv, hv0), mis, flag, abs(cpol - c) / c))
                out[name, T, side] = rows
    return out


def test_polish_removes_the_search_error_and_mismatch_bounds_it():
    tab = polish_table()
    w = [max(r[n][0] for r in tab.values()) for n in range(4)]
    print("error of hv after 0, 1, 2, 3 steps from c (1 +- 2e-6), worst: %.2e %.2e %.2e %.2e; mismatch after 2: %.2e; "
          "error / mismatch at 0 steps: %.3f" % (w[0], w[1], w[2], w[3], max(r[2][1] for r in tab.values()),
                                                max(r[0][0] / r[0][1] for r in tab.values())))
    for key, rows in tab.items():
        assert all(r[2] == 0 for r in rows), key
        assert rows[2][0] <= 1e-12 and rows[3][0] <= 1e-12, key
        assert rows[2][3] <= 1e-14 and rows[2][1] <= 1e-12, key   # the polished c is the root; the certificate says so
        for n in (0, 1):   # the two ratios move apart faster than either errs (1e-14: the rounding floor of both)
            assert rows[n][0] <= rows[n][1] + 1e-14, (key, n)
        assert 1e-6 <= rows[0][0] <= 1e-3, key   # (the error the polish is there for: |d ln hv / d ln c| x 2e-6)


def test_a_step_that_leaves_the_window_falls_back_and_flags():
    m, T = R.MODELS["crust"], 8.0
    c = ROOTS["crust"][1] * (1.0 + 3.0e-4)   # far from the root: the secant's first step goes back by 3e-4 > 1e-5
    hv, mis, cpol, flag = R.ellip(m, T, c, 2)
    assert flag == 1 and cpol == c
    assert (hv, mis) == R.ellip(m, T, c, 0)[:2]
    assert mis > 1e-3


def test_batch_conventions():
    """zero rows for a failed model and a c of 0, NaN and the flag for a water layer"""
    m = R.MODELS["crust"]
    L = len(m[0])
    cols = [np.array([a, a, a]).T for a in m]   # [L, 3]
    cols[2] = cols[2].copy()
    cols[2][0, 2] = 0.0
    vel = np.array([ROOTS["crust"][:2], ROOTS["crust"][:2], ROOTS["crust"][:2]])
    vel[0, 1] = 0.0
    hv, mis, cpol, flag = R.ellip_batch([L, L, L], *cols, R.PERIODS[:2], vel, [0, 1, 0], 2)
    assert hv[0, 0] > 0 and hv[0, 1] == 0 and mis[0, 1] == 0 and cpol[0, 1] == 0 and flag[0] == 0
    assert not hv[1].any() and not mis[1].any() and not cpol[1].any() and flag[1] == 0
    assert np.isnan(hv[2]).all() and np.isnan(mis[2]).all() and np.array_equal(cpol[2], vel[2]) and flag[2] == 1


# ---- the gate on the mismatch ------------------------------------------------------------------------------------------------------
def accepted_mismatch():
    """The largest mismatch of an entry that the tests take as a value: over the cases of tests/test_gpu_swd_ellip.py (0 and 2
    steps, velocities within 2e-6 of the root) every entry of a model without the flag -- except the three of its 5x60 case that
    are handed in as velocities that are no roots (a layer's own S and P velocity, root (1 + 3e-4): mismatch 1.16, 0.93, 4.2e-3;
    with them the rule below gives 100, a gate that fails nothing) --, the polish table from c (1 +- 2e-6) unpolished, and the
    plugin test's unpolished sediment model at 1, 2, 4, 8 s.  -> (the value, where, the three left out)"""
    import test_gpu_swd_ellip as T
    worst, where, left_out = 0.0, None, []
    for name, c in T.build_cases().items():
        for n in (0, 2):
            _, mis, _, flag = c["ref%d" % n]
            for b, k in np.argwhere(np.isfinite(mis) & (mis > 0.0)):
                if c["handmade"][b, k]:
                    if n == 0:
                        left_out.append(float(mis[b, k]))
                elif flag[b] == 0 and mis[b, k] > worst:
                    worst, where = float(mis[b, k]), "%s model %d period %g s, %d steps" % (name, b, c["periods"][k], n)
    for key, rows in polish_table().items():
        if rows[0][1] > worst:
            worst, where = rows[0][1], "polish table %s %g s" % key[:2]
    m, x = R.MODELS["sediment"], [1.0, 2.0, 4.0, 8.0]
    for T_, c in zip(x, R.fundamental_roots(m, x)):
        for side in (-1.0, 1.0):
            mis = R.ellip(m, T_, c * (1.0 + side * 2.0e-6), 0)[1]
            if mis > worst:
                worst, where = mis, "plugin test, sediment %g s" % T_
    return worst, where, sorted(left_out)


def test_gate_constant_follows_its_rule():
    """BH_ELLIP_MISMATCH_MAX = the smallest power of ten that is at least ten times the largest mismatch the tests accept"""
    worst, where, left_out = accepted_mismatch()
    print("largest accepted mismatch %.3e (%s); left out: %s" % (worst, where, left_out))
    assert 1e-5 < worst < 1e-3 and len(left_out) == 3 and left_out[0] > 1e-3
    assert R.MISMATCH_MAX == 10.0 ** math.ceil(math.log10(10.0 * worst)) == 1.0e-2
    with open(os.path.join(REPO, "include", "bh_engine_swd_ellip.h")) as f:
        assert "#define BH_ELLIP_MISMATCH_MAX 1.0e-2 " in f.read()
    from bayhunter_amd import engine as E
    assert E.ELLIP_MISMATCH_MAX == R.MISMATCH_MAX


def test_gate_raises_the_flag_and_leaves_the_values():
    m, T = R.MODELS["crust"], 8.0
    root = ROOTS["crust"][1]
    for off, flag in ((3.0e-4, 0), (3.0e-3, 1)):   # unpolished: mismatch 4e-3 passes, 4e-2 does not
        c = root * (1.0 + off)
        hv, mis, cpol, f = R.ellip(m, T, c, 0)
        assert f == flag and (mis > R.MISMATCH_MAX) == bool(flag) and cpol == c
        assert (hv, mis, cpol, 0) == R.ellip(m, T, c, 0, mismatch_max=math.inf)
    assert R.ellip(m, T, root, 2)[3] == 0


def golden_report():
    """the recorded set of models a chain proposes (tests/golden/ellip_exact.npz) under the gate"""
    from conftest import golden
    g = golden("ellip_exact.npz")
    G = R.MISMATCH_MAX
    ok = g["noexact"] == 0
    prior = ok & (g["kind"] == 0)[:, None]
    lines = ["recorded set: %d models x %d periods (%g-%g s), %d pairs with a %d-digit value, %d of them prior-drawn"
             % (g["c"].shape + (g["periods"][0], g["periods"][-1], ok.sum(), int(g["digits"][ok].min()), prior.sum()))]
    d = np.abs(g["c"] / np.where(ok, g["cstar"], 1.0) - 1.0)
    sens = np.abs(g["hv0"] / np.where(ok, g["hvstar"], 1.0) - 1.0) / np.where(d > 1e-12, d, np.nan)
    for name, sel in (("two steps converge (mismatch < 1e-9)", ok & (g["mis2"] < 1e-9)), ("they do not (mismatch > 1e-2)", ok & (g["mis2"] > 1e-2))):
        lines.append("  |d ln hv / d ln c| where %s, %d pairs: %.2g to %.2g" % (name, sel.sum(), np.nanmin(sens[sel]), np.nanmax(sens[sel])))
    edges = [0.0] + [10.0 ** e for e in range(-15, 2)] + [np.inf]
    for n in (0, 2):
        mis, flag, hv = g["mis%d" % n], g["flag%d" % n], g["hv%d" % n]
        ang = np.abs(np.arctan(hv) - np.arctan(g["hvstar"]))
        acc = ok & (flag == 0)
        lines.append("nsteps = %d: accepted %d of %d; worst |atan hv - atan hv*| among accepted %.2e (bound %.0e); largest accepted "
                     "mismatch %.2e; prior-drawn pairs the gate or the polish fails: %d of %d (%.1f %%)"
                     % (n, acc.sum(), ok.sum(), ang[acc].max(), G, mis[acc].max(), (prior & ~acc).sum(), prior.sum(),
                        100.0 * (prior & ~acc).sum() / prior.sum()))
        h = np.histogram(mis[ok], bins=edges)[0]
        lines.append("  mismatch histogram (upper edge: count): " + ", ".join(
            "%s: %d" % ("inf" if np.isinf(e) else "%.0e" % e, c) for e, c in zip(edges[1:], h) if c))
        top = np.sort(mis[acc])[-4:]
        lines.append("  the four largest accepted: " + ", ".join("%.2e" % v for v in top)
                     + ("  (within a decade of the constant: %d)" % (mis[acc] > 0.1 * G).sum()))
    return lines


def accuracy_report():
    tab = polish_table()
    cf_worst, cf_root, cf = closed_form_worst()
    lines = ["Rayleigh ellipticity: the restatement (tests/ellip_ref.py) on the CPU, float64; models %s, periods %s s"
             % (", ".join(R.MODELS), ", ".join("%g" % T for T in R.PERIODS)),
             "ODE route, its two ratios against each other, worst of 24: %.2e" % max(rel(o1, o2) for _, o1, o2 in ODE.values()),
             "restatement against the ODE route, worst of 24: %.2e" % max(rel(abs(hv), abs(o1)) for hv, o1, _ in ODE.values()),
             "homogeneous stack against the closed form %.14f: %.2e" % (cf, cf_worst)]
    for n in range(4):
        lines.append("from c (1 +- 2e-6), nsteps = %d: error of hv <= %.2e, mismatch <= %.2e, error / mismatch <= %.3f"
                     % (n, max(r[n][0] for r in tab.values()), max(r[n][1] for r in tab.values()),
                        max(r[n][0] / max(r[n][1], 1e-300) for r in tab.values())))
    worst, where, left_out = accepted_mismatch()
    lines.append("the gate: largest mismatch of an entry the tests take as a value %.3e (%s); BH_ELLIP_MISMATCH_MAX = %.0e, the "
                 "smallest power of ten >= 10 x that" % (worst, where, R.MISMATCH_MAX))
    lines.append("  left out of that maximum, handed in as velocities that are no roots (unpolished mismatch): %s -- with them the rule "
                 "gives 100, a gate that fails nothing" % ", ".join("%.3g" % v for v in left_out))
    lines += golden_report()
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    with open(os.path.join(REPO, "profiles", "swd_ellip_accuracy.txt"), "w") as f:
        f.write(accuracy_report())
    print(accuracy_report())
