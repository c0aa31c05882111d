"""The Rayleigh ellipticity on the GPU (include/bh_engine_swd_ellip.h; bayhunter_amd/csrc/swd_ellip.hip) against its plain-Python
restatement (tests/ellip_ref.py), bit for bit; end to end behind the engine's own search against the closed form of a half-space
and the restatement at its own bisected root; the plugin, the joint target and a short inversion.

The end-to-end bounds (1e-10) are three orders over what the polish leaves on the CPU (3e-14, tests/test_ellip_ref.py) and four
under what it removes (|d ln hv / d ln c| x the 2e-6 the default search promises)."""
import math

import numpy as np
import pytest

import bayhunter_amd as bh
import ellip_ref as R

pytestmark = pytest.mark.gpu

DELTAS = (2.0e-6, -2.0e-6, 0.0, 5.0e-7, -1.0e-6)   # how far from the root the velocities handed in lie


def grad_model(n, i=0):
    """n layers, velocities rising with depth"""
    vs = 2.6 + 0.02 * i + (4.5 - 2.6) * np.arange(n) / max(n - 1, 1)
    h = np.r_[np.full(n - 1, 2.0 + 0.3 * i), 0.0]
    vp = vs * 1.75
    return h, vp, vs, vp * 0.32 + 0.77


def named(name):
    return [np.array(a) for a in R.MODELS[name]]


DEEP50 = (np.array([50.0, 10.0, 0.0]), np.array([6.1, 6.9, 8.0]), np.array([3.5, 3.9, 4.5]), np.array([2.7, 2.95, 3.3]))


def build_case(models, periods, special=None):
    """-> dict: packed layer-major models, vel [B, K] near every model's fundamental roots (special(b, k, model, root) may replace
    an entry), err [B]"""
    nlay, h, vp, vs, rho = bh.pack_models(models)
    B, K = len(models), len(periods)
    vel = np.zeros((B, K))
    handmade = np.zeros((B, K), dtype=bool)   # entries that `special` replaced: velocities that are no roots
    for b, m in enumerate(models):
        rm = R.round_model(*m)
        if not rm[2][0] > 0.0:   # a water layer has no restated root: any velocity will do
            vel[b] = 1.4
            continue
        for k, c in enumerate(R.fundamental_roots(rm, periods)):
            vel[b, k] = c * (1.0 + DELTAS[(b + k) % len(DELTAS)])
            if special is not None:
                s = special(b, k, rm, c)
                vel[b, k] = vel[b, k] if s is None else s
                handmade[b, k] = s is not None
    return dict(handmade=handmade, nlay=nlay, h=h, vp=vp, vs=vs, rho=rho, periods=np.asarray(periods, dtype=float), vel=vel,
                err=np.zeros(B, dtype=np.int32))


def branches(case):
    """which arms of the layer terms (swd_common.h: layer_products) the case's evaluations at the velocities handed in reach"""
    seen = set()
    for b in range(case["vel"].shape[0]):
        n = int(case["nlay"][b])
        d, a, s, _ = R.round_model(case["h"][:n, b], case["vp"][:n, b], case["vs"][:n, b], case["rho"][:n, b])
        for k, T in enumerate(case["periods"]):
            c = case["vel"][b, k]
            if not c > 0.0 or case["err"][b] != 0 or not s[0] > 0.0:
                continue
            om = R.TWOPI / T
            wv = om / c
            for m in range(n - 1):
                xka, xkb = om / a[m], om / s[m]
                ra, rb = math.sqrt((wv + xka) * abs(wv - xka)), math.sqrt((wv + xkb) * abs(wv - xkb))
                seen.add("P prop" if wv < xka else "P eq" if wv == xka else "P evan")
                seen.add("S prop" if wv < xkb else "S eq" if wv == xkb else "S evan")
                if wv > xka and ra * d[m] >= 16.0:
                    seen.add("p >= 16")
                if wv > xkb and rb * d[m] >= 16.0:
                    seen.add("q >= 16")
                if wv > xka and wv > xkb and ra * d[m] + rb * d[m] >= 60.0:
                    seen.add("exa >= 60")
    return seen


def special_big(b, k, rm, root):
    if (b, k) == (0, 3):
        return 0.0                       # no root at this period: a zero entry
    if b == 2 and k == 5:
        return rm[2][1]                  # c == (double)(float)vs of layer 1: the equality arm of the S terms
    if b == 2 and k == 6:
        return rm[1][0]                  # c == (double)(float)vp of the sediment: the equality arm of the P terms
    if b == 3 and k == 7:
        return root * (1.0 + 3.0e-4)     # the secant's first step goes back by 3e-4 c: out of the window
    return None


def build_cases():
    """the cases of the bitwise tests with the restatement's results (CPU; tests/test_ellip_ref.py derives the gate's constant
    from them)"""
    out = {}
    out["1x1"] = build_case([named("crust")], [8.0])
    out["3x7"] = build_case([named("crust"), named("sediment"), named("lvz")], [1.0, 2.0, 3.5, 6.0, 11.0, 19.0, 33.0])
    big = build_case([named("crust"), named("poisson"), named("sediment"), named("lvz"), DEEP50], np.linspace(1.0, 40.0, 60),
                     special_big)
    big["err"][1] = 1                     # a model whose dispersion search failed: a zero row
    out["5x60"] = big
    ragged = [grad_model(n, n) for n in range(2, 14)]            # 2 .. 13 layers, 12 models x 6 periods: the first wavefront
    w = [a.copy() for a in grad_model(6, 1)]                     # holds models of 2 .. 12 layers
    w[2][0] = 0.0                                                # ... and a water layer: not supported, NaN and the flag
    out["ragged"] = build_case(ragged + [tuple(w)], [1.5, 3.0, 6.0, 12.0, 24.0, 40.0])
    for name, c in out.items():
        for nsteps in (0, 2):
            c["ref%d" % nsteps] = R.ellip_batch(c["nlay"], c["h"], c["vp"], c["vs"], c["rho"], c["periods"], c["vel"], c["err"], nsteps)
    return out


@pytest.fixture(scope="module")
def cases():
    return build_cases()


def test_cases_reach_every_arm_of_the_layer_terms(cases):
    seen = set()
    for c in cases.values():
        seen |= branches(c)
    assert seen == {"P prop", "P eq", "P evan", "S prop", "S eq", "S evan", "p >= 16", "q >= 16", "exa >= 60"}
    assert "exa >= 60" in branches(cases["5x60"]) and cases["5x60"]["periods"][0] == 1.0   # the 50 km layer at T = 1 s
    big = cases["5x60"]
    hv0, _, _, flag0 = big["ref0"]
    hv2, mis2, cpol2, flag2 = big["ref2"]
    # unpolished, the sediment model's two velocities that are a layer's own (no roots: mismatch 1.16 and 0.93) meet the gate on
    # the mismatch; root (1 + 3e-4) (mismatch 4.2e-3) passes it
    assert list(flag0) == [0, 0, 1, 0, 0]
    assert big["ref0"][1][2, 5] > 0.9 and big["ref0"][1][2, 6] > 0.9 and 1e-3 < big["ref0"][1][3, 7] <= R.MISMATCH_MAX
    assert list(flag2) == [0, 0, 1, 1, 0]                        # the velocities that are no roots; the step out of the window
    assert cpol2[3, 7] == big["vel"][3, 7] and hv2[3, 7] == hv0[3, 7] and mis2[3, 7] > 1e-3   # ... fell back to the unpolished value
    assert hv2[0, 3] == 0 and cpol2[0, 3] == 0 and not hv2[1].any() and not cpol2[1].any()
    ok = np.ones_like(hv2, dtype=bool)
    ok[0, 3] = ok[1, :] = ok[2, 5:7] = ok[3, 7] = False
    assert np.all(mis2[ok] <= 1e-11) and np.all(np.abs(cpol2[ok] / big["vel"][ok] - 1.0) <= 3e-6)   # polished entries are roots
    rag = cases["ragged"]
    assert list(rag["nlay"][:12]) == list(range(2, 14)) and rag["vel"].shape == (13, 6)
    assert np.isnan(rag["ref2"][0][12]).all() and rag["ref2"][3][12] == 1 and not rag["ref2"][3][:12].any()


@pytest.mark.parametrize("layout", ["layer_major", "model_major"])
@pytest.mark.parametrize("nsteps", [0, 2])
@pytest.mark.parametrize("name", ["1x1", "3x7", "5x60", "ragged"])
def test_kernel_returns_the_restatements_bits(engine, cases, name, nsteps, layout):
    c = cases[name]
    arrs = [c[k] if layout == "layer_major" else np.ascontiguousarray(c[k].T) for k in ("h", "vp", "vs", "rho")]
    out = engine.swd_ellip(c["nlay"], *arrs, c["periods"], vel=c["vel"], err=c["err"], nsteps=nsteps, layout=layout)
    hv, mis, cpol, flag = c["ref%d" % nsteps]
    assert np.array_equal(out["vel"], c["vel"]) and np.array_equal(out["err"], c["err"])   # read, not written
    assert np.array_equal(out["flag"], flag)
    assert R.same_bits(out["c"], cpol)
    assert R.same_bits(out["hv"], hv)
    assert R.same_bits(out["mismatch"], mis)


def test_device_entry_and_optional_outputs(engine, cases):
    """swd_ellip_dev on torch tensors, mismatch and cpol left out: the same hv and flag"""
    import torch
    c = cases["3x7"]
    dev = torch.device("cuda", engine.device)
    t = {k: torch.as_tensor(c[k], device=dev) for k in ("nlay", "h", "vp", "vs", "rho", "periods", "vel", "err")}
    B, K = c["vel"].shape
    hv = torch.full((B, K), 7.0, dtype=torch.float64, device=dev)
    flag = torch.full((B,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    engine.swd_ellip_dev(B, c["h"].shape[0], t["nlay"].data_ptr(), t["h"].data_ptr(), t["vp"].data_ptr(), t["vs"].data_ptr(),
                         t["rho"].data_ptr(), B, 1, K, t["periods"].data_ptr(), t["vel"].data_ptr(), t["err"].data_ptr(),
                         hv.data_ptr(), flag.data_ptr(), have_vel=True, nsteps=2)
    engine.synchronize()
    assert R.same_bits(hv.cpu().numpy(), c["ref2"][0]) and np.array_equal(flag.cpu().numpy(), c["ref2"][3])


def test_argument_errors(engine, cases):
    c = cases["1x1"]
    E = bh.EngineError
    with pytest.raises(E, match="nsteps must be 0..3"):
        engine.swd_ellip(c["nlay"], c["h"], c["vp"], c["vs"], c["rho"], c["periods"], nsteps=4)
    with pytest.raises(E, match="K must be 1..60"):
        engine.swd_ellip(c["nlay"], c["h"], c["vp"], c["vs"], c["rho"], np.linspace(1, 40, 61))
    with pytest.raises(E, match="K must be 1..60"):
        engine.swd_ellip(c["nlay"], c["h"], c["vp"], c["vs"], c["rho"], np.zeros(0))
    with pytest.raises(E, match="null argument"):
        engine.swd_ellip_dev(1, 4, None, None, None, None, None, 1, 1, 1, None, None, None, None, None)
    with pytest.raises(ValueError, match="vel and err go together"):
        engine.swd_ellip(c["nlay"], c["h"], c["vp"], c["vs"], c["rho"], c["periods"], vel=c["vel"])


# ---- end to end: the engine's own search first ------------------------------------------------------------------------------------
SEARCHES = (("fast", "fast"), ("reference", "exact"))   # the engine's defaults; the reference's sequence and arithmetic


def four_models():
    names = list(R.MODELS)
    nlay, h, vp, vs, rho = bh.pack_models([named(n) for n in names])
    return names, nlay, h, vp, vs, rho


@pytest.fixture(scope="module")
def end_to_end(engine):
    names, nlay, h, vp, vs, rho = four_models()
    out = {}
    for search, arith in SEARCHES:
        with engine.searching(search), engine.computing(arith):
            out[search] = engine.swd_ellip(nlay, h, vp, vs, rho, R.PERIODS)
    roots = np.array([R.fundamental_roots(R.MODELS[n], R.PERIODS) for n in names])
    ref = np.array([[R.ellip(R.MODELS[n], T, c, 0)[0] for T, c in zip(R.PERIODS, roots[i])] for i, n in enumerate(names)])
    return names, out, roots, ref


def test_homogeneous_stack_gives_the_closed_form(end_to_end):
    names, out, _, _ = end_to_end
    m = R.MODELS["poisson"]
    cf = float(R.halfspace_hv(m[1][0], m[2][0]))
    i = names.index("poisson")
    for search, _ in SEARCHES:
        o = out[search]
        worst = np.max(np.abs(o["hv"][i] - cf))
        print("homogeneous stack, %s search: |hv - closed form| <= %.2e" % (search, worst))
        assert o["err"][i] == 0 and o["flag"][i] == 0
        assert worst <= 1e-10


def test_four_models_agree_with_the_restatement_at_its_bisected_root(end_to_end):
    names, out, roots, ref = end_to_end
    for search, _ in SEARCHES:
        o = out[search]
        assert not o["err"].any() and not o["flag"].any()
        assert np.max(np.abs(o["vel"] / roots - 1.0)) <= 1e-5           # the same root: the fundamental mode
        worst = np.max(np.abs(o["hv"] / ref - 1.0))
        print("four models, %s search: hv against the restatement at its root <= %.2e; c <= %.2e; mismatch <= %.2e"
              % (search, worst, np.max(np.abs(o["c"] / roots - 1.0)), o["mismatch"].max()))
        assert worst <= 1e-10
        assert np.array_equal(np.sign(o["hv"]), np.sign(ref))
    a, b = out["fast"], out["reference"]
    dv = np.max(np.abs(a["vel"] / b["vel"] - 1.0))
    dh = np.max(np.abs(a["hv"] / b["hv"] - 1.0))
    print("the two searches: vel differs by <= %.2e, hv by <= %.2e" % (dv, dh))
    assert dv <= 2e-6 and dh <= 1e-10


# ---- the plugin -------------------------------------------------------------------------------------------------------------------
def test_surfellip_run_model_contract(engine):
    m = named("sediment")
    x = np.array([1.0, 2.0, 4.0, 8.0])
    roots = R.fundamental_roots(R.MODELS["sediment"], x)
    ref = np.array([R.ellip(R.MODELS["sediment"], T, c, 0)[0] for T, c in zip(x, roots)])
    assert list(ref > 0) == [True, False, True, True]            # prograde at T = 2 s
    p = bh.SurfEllip(x, engine=engine)
    xo, y = p.run_model(*m)
    assert xo is p.obsx and y.shape == (4,)
    assert np.all(y > 0) and np.max(np.abs(y / np.abs(ref) - 1.0)) <= 1e-10   # the amplitude ratio
    p.set_modelparams(signed=True)
    ys = p.run_model(*m)[1]
    assert np.array_equal(np.abs(ys), y) and ys[1] < 0 and np.array_equal(np.sign(ys), np.sign(ref))
    p.set_modelparams(ratio="zh")
    assert np.array_equal(p.run_model(*m)[1], 1.0 / ys)
    p.set_modelparams(nsteps=0, ratio="hv")                      # unpolished: the search's velocity as it is
    y0 = p.run_model(*m)[1]
    assert 0 < np.max(np.abs(y0 / ref - 1.0)) <= 1e-3
    # a model without a root: (nan, nan), and a NaN row with err in a batch
    bad = [a.copy() for a in m]
    bad[1][1] = 200.0
    assert all(np.isnan(v) for v in p.run_model(*bad))
    nlay, h, vp, vs, rho = bh.pack_models([m, bad, named("crust")])
    _, yb, err = p.run_models(nlay, h, vp, vs, rho)
    assert list(err) == [0, 1, 0] and np.isnan(yb[1]).all() and np.array_equal(yb[0], y0) and np.isfinite(yb[2]).all()


# ---- the joint target -------------------------------------------------------------------------------------------------------------
X = np.array([2.0, 4.0, 8.0, 12.0, 20.0, 30.0])


def joint(engine):
    td = bh.RayleighDispersionPhase(X, 3.0 + 0.03 * X)
    te = bh.RayleighEllipticity(X, 0.9 + 0.0 * X)
    td.set_noise_law("exp")
    te.set_noise_law("nocorr")
    return bh.JointTarget([td, te], engine=engine), td, te


def test_joint_target_batches_the_ellipticity(engine):
    jt, td, te = joint(engine)
    bad = [a.copy() for a in named("crust")]
    bad[1][2] = 200.0
    nlay, h, vp, vs, rho = bh.pack_models([named("crust"), named("sediment"), bad, named("lvz")])
    noise = np.tile([0.3, 0.05, 0.0, 0.1], (4, 1))
    logL, misfits, err, ymod = jt.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True)
    _, yd, ed = td.moddata.plugin.run_models(nlay, h, vp, vs, rho)
    _, ye, ee = te.moddata.plugin.run_models(nlay, h, vp, vs, rho)
    want = np.hstack([np.nan_to_num(yd), np.nan_to_num(ye)])
    assert R.same_bits(ymod, want)
    ref = engine.loglike_batch(want, noise, np.array([ed, ee]))
    assert R.same_bits(logL, ref[0]) and R.same_bits(misfits, ref[1]) and np.array_equal(err, ref[2])
    assert list(err != 0) == [False, False, True, False] and logL[2] == -1e15 and np.all(np.isfinite(logL[[0, 1, 3]]))
    o = engine.swd_ellip(nlay, h, vp, vs, rho, X)
    assert np.array_equal(ymod[[0, 1, 3], X.size:], np.abs(o["hv"][[0, 1, 3]]))
    # one model, the reference's signature
    m = named("sediment")
    jt.evaluate(m[0], m[1], m[2], noise[0], rho=m[3])
    assert jt.proposallikelihood == logL[1] and np.array_equal(jt.proposalmisfits, misfits[1])
    assert np.array_equal(te.moddata.x, X) and np.array_equal(te.moddata.y, ymod[1, X.size:])
    assert np.array_equal(td.moddata.y, ymod[1, :X.size])
    jt.evaluate(bad[0], bad[1], bad[2], noise[0], rho=bad[3])
    assert jt.proposallikelihood == -1e15


def test_short_inversion_with_the_ellipticity(engine):
    m = named("crust")
    pd = bh.SurfDisp(X, "rdispph", engine=engine)
    pe = bh.SurfEllip(X, engine=engine)
    td = bh.RayleighDispersionPhase(X, pd.run_model(*m)[1])
    te = bh.RayleighEllipticity(X, pe.run_model(*m)[1])
    priors = {"vs": (2.0, 5.0), "z": (0, 60), "layers": (1, 6), "vpvs": 1.73, "swdnoise_corr": 0.0, "swdnoise_sigma": (1e-3, 0.1),
              "ellnoise_corr": 0.0, "ellnoise_sigma": (1e-3, 0.2)}
    init = {"iter_burnin": 100, "iter_main": 100, "propdist": (0.025, 0.025, 0.015, 0.005, 0.005), "acceptance": (40, 45)}
    batch = bh.ChainBatch(bh.JointTarget([td, te], engine=engine), [11, 12, 13, 14], init, priors).run()
    assert batch.noisepriors == [0.0, (1e-3, 0.1), 0.0, (1e-3, 0.2)]
    for c in batch.chains:
        likes = np.asarray(c.likes, dtype=float)
        assert likes.size >= 1 and np.all(np.isfinite(likes)) and np.all(likes > -1e14)
        assert c.accepted.sum() > 0
