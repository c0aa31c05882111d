"""The recorded set tests/golden/ellip_exact.npz (tests/golden/gen_ellip_golden.py): the Rayleigh ellipticity of models of the kind a
chain proposes, from a 110-digit route that shares no formula with the library (tests/ellip_exact.py).  No GPU: that the file comes
from its generator, what it must contain to be worth its place, and what the restatement (tests/ellip_ref.py -- the kernel's bits,
tests/test_gpu_ellip_exact.py) makes of it with and without the gate on the mismatch.

Bounds.  1e-15 for the re-derivation: the stored values are float64 roundings (<= 1.2e-16) of numbers known to 80 digits.  G, the
safety bound on the angle, is the gate's constant: for hv* between hv and hv_alt, |atan hv - atan hv*| <= |atan hv - atan hv_alt|
<= |hv - hv_alt| / (1 + min(hv^2, hv_alt^2)) on one side of zero, <= mismatch |hv| / (1 + ...) <= mismatch.  1e-12 |hv| in the
certificate is the rounding floor of the two float64 ratios (tests/test_ellip_ref.py: <= 1.2e-14 on the well-behaved stacks)."""
import math

import numpy as np
import pytest

import ellip_exact as X
import ellip_ref as R
from conftest import golden

G = R.MISMATCH_MAX


@pytest.fixture(scope="module")
def gold():
    return golden("ellip_exact.npz")


def model_of(g, b):
    n = int(g["nlay"][b])
    return R.round_model(*[g[a][:n, b] for a in ("h", "vp", "vs", "rho")])


def classes(g):
    ok = g["noexact"] == 0
    return ok, ok & (g["mis2"] < 1e-9), ok & (g["mis2"] > 1e-2)


def test_the_set_holds_what_it_is_there_for(gold):
    g = gold
    ok, well, trapped = classes(g)
    print("pairs with an exact value %d, mismatch after two steps below 1e-9: %d, above 1e-2: %d" % (ok.sum(), well.sum(), trapped.sum()))
    assert g["c"].shape == (71, 8) and g["periods"][0] == 0.5 and g["periods"][-1] == 40.0
    assert ok.sum() >= 250 and trapped.sum() >= 30 and well.sum() >= 200
    assert list(np.flatnonzero(g["err"])) == [70] and g["noexact"][70].all() and g["noexact"][69].all()   # no root; under water
    assert np.all(g["c"][ok] < np.array([g["vs"][g["nlay"][b] - 1, b] for b in range(71)])[:, None].repeat(8, 1)[ok])
    assert np.all(np.abs(g["cstar"][ok] / g["c"][ok] - 1.0) <= 1e-5)


def dozen(g):
    """six pairs of each class from six different models each -- those whose exact evaluation costs least (few layers, long
    periods, the first rung of the ladder), so the test takes seconds"""
    _, well, trapped = classes(g)
    out = []
    for cls in (well, trapped):
        idx = [tuple(i) for i in np.argwhere(cls & (g["digits"] == X.LADDER[0][0]))]
        idx.sort(key=lambda bk: (g["nlay"][bk[0]] / g["periods"][bk[1]], bk))
        seen = []
        for b, k in idx:
            if b not in [s[0] for s in seen]:
                seen.append((b, k))
        out += seen[:6]
    assert len(out) == 12
    return out


def test_stored_exact_values_come_from_the_generator(gold):
    g = gold
    for b, k in dozen(g):
        cstar, hvstar, _ = X.ellipticity(X.exact_model(*model_of(g, b)), float(g["periods"][k]), float(g["c"][b, k]))
        assert abs(float(cstar) / g["cstar"][b, k] - 1.0) <= 1e-15, (b, k)
        assert abs(float(hvstar) / g["hvstar"][b, k] - 1.0) <= 1e-15, (b, k)


def test_stored_restatement_is_the_restatement(gold):
    g = gold
    for n in (0, 2):
        for b in range(0, 71, 3):
            for k in range(8):
                if g["err"][b] == 0 and g["c"][b, k] > 0.0:
                    got = R.ellip(model_of(g, b), float(g["periods"][k]), float(g["c"][b, k]), n)
                    want = [g[key % n][b, k] for key in ("hv%d", "mis%d", "cpol%d", "flag%d")]
                    assert R.same_bits(np.array(got[:3]), np.array(want[:3])) and got[3] == want[3], (n, b, k)


def angle(hv, hvstar):
    return np.abs(np.arctan(hv) - np.arctan(hvstar))


def test_gated_restatement_is_safe_and_the_ungated_one_is_not(gold):
    """With the gate no accepted entry is off by more than G in angle; without it (the flag of the polish alone) entries that are
    wrong by O(1) are accepted -- what a fused call fed to the likelihood."""
    g = gold
    ok = g["noexact"] == 0
    for n in (0, 2):
        hv, mis, flag = g["hv%d" % n], g["mis%d" % n], g["flag%d" % n]
        old = np.zeros_like(flag)
        for b, k in np.argwhere(ok):
            old[b, k] = R.ellip(model_of(g, b), float(g["periods"][k]), float(g["c"][b, k]), n, mismatch_max=math.inf)[3]
        ang = angle(hv, g["hvstar"])
        acc, acc_old = ok & (flag == 0), ok & (old == 0)
        unsafe_old = acc_old & (ang > G)
        print("nsteps %d: accepted %d of %d, worst angle %.2e; without the gate accepted %d, of them off by more than G: %d, worst %.3f"
              % (n, acc.sum(), ok.sum(), ang[acc].max(), acc_old.sum(), unsafe_old.sum(), ang[acc_old].max()))
        assert np.all(ang[acc] <= G)
        if n == 2:   # (unpolished, the certificate misses one accepted pair by 2 %: the last test of this file)
            assert np.all(np.abs(hv - g["hvstar"])[acc] <= (mis * np.abs(hv) + 1e-12 * np.abs(hv))[acc])
        assert np.array_equal(flag[ok] != 0, (old[ok] != 0) | ~(mis[ok] <= G))       # the gate adds exactly mismatch > G
        assert unsafe_old.sum() >= 30 and ang[acc_old].max() > 0.5
        assert np.all(flag[acc & (g["mis2"] < 1e-9)] == 0)


def test_where_the_certificate_does_not_hold(gold):
    """|hv - hv*| <= mismatch |hv| says that hv* lies between the two expressions.  It holds on all pairs of the set but two.

    1.  m(0,2) m(1,3) - m(0,3) m(1,2) = -m(0,1) m(2,3): the two expressions are equal at a root of the traction minor m(2,3) AND
    at a root of the displacement minor m(0,1).  Pair (18, 3): the secant of the polish stalls (e0 is 1.0 at both of its points) a
    relative 1e-6 above the root, where m(0,1) changes sign -- mismatch 0.04 with hv = -1.36 against 0.82 at the root.  A small
    mismatch is necessary for a root, not sufficient; the gate fails this entry.
    2.  Unpolished, pair (29, 5) -- five layers, 15 s, c 6.5e-7 below the root -- has both expressions on the same side of hv*:
    |hv - hv*| = 2.816e-6 |hv| against a mismatch of 2.758e-6, 2 % over.  The entry is accepted and right to 3e-6; the statement
    "off the root the two move in opposite directions" is a tendency, not a law.  After two steps the pair satisfies it."""
    g = gold
    ok = g["noexact"] == 0

    def broken(n):
        hv, mis = g["hv%d" % n], g["mis%d" % n]
        return [tuple(i) for i in np.argwhere(ok & ~(np.abs(hv - g["hvstar"]) <= mis * np.abs(hv) + 1e-12 * np.abs(hv)))]

    assert broken(2) == [(18, 3)] and g["flag2"][18, 3] == 1 and 0.01 < g["mis2"][18, 3] < 0.1
    m, T, c = X.exact_model(*model_of(g, 18)), float(g["periods"][3]), float(g["cpol2"][18, 3])
    lo, hi = X.Surface(m, T, c * (1 - 2e-7)), X.Surface(m, T, c * (1 + 2e-7))
    assert lo.minor(0, 1) * hi.minor(0, 1) < 0 and lo.minor(2, 3) * hi.minor(2, 3) > 0
    assert broken(0) == [(29, 5)] and g["flag0"][29, 5] == 0
    err = abs(g["hv0"][29, 5] - g["hvstar"][29, 5]) / abs(g["hv0"][29, 5])
    assert g["mis0"][29, 5] < err <= 1.03 * g["mis0"][29, 5] and err <= 3e-6
