"""The Rayleigh ellipticity in the fused call and the device chains (include/bh_engine_ellip_target.h) against the route that
exists beside it: `RayleighEllipticity(fused=False)`, whose synthetics come from `SurfEllip.run_models` (bh_swd_batch, then
bh_swd_ellip) and go to bh_loglike_batch.  Under the reference's search the two routes give the same bits; under the engine's
default search the same failures and y within 1e-12, the bound tests/test_ellip_ref.py asserts for two polish steps whichever
search produced c."""
import ctypes as C

import numpy as np
import pytest

import bayhunter_amd as bh
from bayhunter_amd.Models import Model
from bayhunter_amd.device_chains import DeviceChains
from test_gpu_swd_ellip import grad_model, named

pytestmark = pytest.mark.gpu

POLISH_BOUND = 1e-12                                     # tests/test_ellip_ref.py: rows[2][0] <= 1e-12
X7 = np.array([1.0, 2.0, 3.5, 6.0, 11.0, 19.0, 33.0])
X7_OTHER = np.array([1.5, 2.5, 4.0, 7.0, 12.0, 21.0, 30.0])
XRF = np.linspace(-5.0, 35.0, 201)
B70, WATER, NOROOT, HALFSPACE, SEDIMENT = 70, 36, 5, 12, 40


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def seventy():
    """70 models of 1 .. 12 layers in arrays of 13 rows; with 7 periods model 36 owns lanes 252 .. 258, the last four of the first
    workgroup and the first three of the second: it is the one under a kilometre of water -- the search finds its roots, and every
    lane of the ellipticity raises the flag"""
    models = [grad_model(1 + i % 12, i % 7) for i in range(B70)]
    c = named("crust")
    models[WATER] = (np.r_[1.0, c[0]], np.r_[1.5, c[1]], np.r_[0.0, c[2]], np.r_[1.03, c[3]])
    bad = [a.copy() for a in named("sediment")]
    bad[1][1] = 200.0                                    # the dispersion search fails on it (tests/test_gpu_swd_ellip.py)
    models[NOROOT] = tuple(bad)
    models[SEDIMENT] = tuple(named("sediment"))          # prograde at T = 2 s
    models[41] = tuple(named("lvz"))
    assert len(models[HALFSPACE][0]) == 1
    nlay, h, vp, vs, rho = bh.pack_models(models, Lmax=13)
    assert sorted(set(nlay)) == list(range(1, 13)) and h.shape == (13, B70)
    return nlay, h, vp, vs, rho


MODELS70 = seventy()


def target(cls, x, y, law, yerr=None, **kw):
    t = cls(x, y, yerr=yerr, **kw)
    t.set_noise_law(law)
    return t


def ellip(x, fused, law="nocorr", yerr=None, **params):
    t = target(bh.RayleighEllipticity, x, 0.75 + 0.01 * x, law, yerr=yerr, fused=fused)
    if params:
        t.moddata.plugin.set_modelparams(**params)
    return t


def phase(x=X7, law="nocorr", yerr=None, cls=bh.RayleighDispersionPhase):
    return target(cls, x, 3.0 + 0.03 * x, law, yerr=yerr)


def prf():
    t = target(bh.PReceiverFunction, XRF, 0.05 * np.exp(-0.5 * (XRF / 1.5) ** 2), "exp")
    t.moddata.plugin.set_modelparams(gauss=1.0, p=6.4)
    return t


def pair(engine, others, x=X7, law="nocorr", yerr=None, first=True, **params):
    """the same target list twice: with the ellipticity fused, and as it was"""
    out = []
    for fused in (True, False):
        ts = list(others()) if callable(others) else []
        e = ellip(x, fused, law, yerr, **params)
        out.append(bh.JointTarget(ts + [e] if first else [e] + ts, engine=engine))
    return out


def noise_for(jt, B):
    row = []
    for t in jt.targets:
        row += [0.4 if t.law() == "exp" else 0.0, 0.07 if isinstance(t, bh.RayleighEllipticity) else 0.05]
    return np.tile(np.array(row), (B, 1))


def assert_same(got, ref, what, exact=True, ell_cols=None):
    (l1, m1, e1, y1), (l0, m0, e0, y0) = got, ref
    assert np.array_equal(e1, e0), what
    ok = e0 == 0
    if exact:
        assert np.array_equal(bits(l1), bits(l0)) and np.array_equal(bits(m1), bits(m0)), what
        assert np.array_equal(bits(y1[ok]), bits(y0[ok])), what
    else:
        assert np.all(l1[~ok] == -1e15) and np.array_equal(np.isfinite(l1[ok]), np.isfinite(l0[ok])), what   # (a half-space's receiver function is no number)
        a, b = y1[ok][:, ell_cols], y0[ok][:, ell_cols]
        worst = np.max(np.abs(a - b) / np.abs(b))
        print("%s: y of the two routes differs by <= %.2e relative" % (what, worst))
        assert worst <= POLISH_BOUND, what
    return ok


def both_searches(engine):
    """the reference's search: bits; the default one at 32 trials per round: the same failures, y within the polish's bound"""
    yield "reference", True, (engine.searching("reference"), engine.computing("exact"), engine.trying(None))
    yield "fast", False, (engine.searching("fast"), engine.computing("fast"), engine.trying(32))


# ---- 5: the fused call against the existing route ---------------------------------------------------------------------------------
@pytest.mark.parametrize("law", ["nocorr", "exp"])
def test_fused_call_gives_the_existing_routes_results(engine, law):
    nlay, h, vp, vs, rho = MODELS70
    yerr = None if law == "nocorr" else 0.02 + 0.001 * X7
    jf, j0 = pair(engine, lambda: [phase(X7, law, yerr)], law=law, yerr=yerr)
    noise = noise_for(jf, B70)
    cols = slice(X7.size, 2 * X7.size)
    for name, exact, ctx in both_searches(engine):
        with ctx[0], ctx[1], ctx[2]:
            for layout in ("layer_major", "model_major"):
                arrs = [a if layout == "layer_major" else np.ascontiguousarray(a.T) for a in (h, vp, vs, rho)]
                ref = j0.evaluate_batch(nlay, arrs[0], arrs[1], arrs[2], noise, rho=arrs[3], layout=layout, want_ymod=True)
                got = jf.evaluate_batch(nlay, arrs[0], arrs[1], arrs[2], noise, rho=arrs[3], layout=layout, want_ymod=True)
                ok = assert_same(got, ref, "%s %s %s" % (law, name, layout), exact, cols)
                three = jf.evaluate_batch(nlay, arrs[0], arrs[1], arrs[2], noise, rho=arrs[3], layout=layout)   # (no synthetics asked for)
                assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(three[:2], got[:2])) and np.array_equal(three[2], got[2])
            assert list(np.flatnonzero(~ok)) == sorted([NOROOT, WATER]), name
            assert ok[HALFSPACE] and np.all(got[3][HALFSPACE, cols] > 0)
            assert got[0][WATER] == -1e15 and np.all(got[1][WATER] == 1e15)
            if exact:   # the device entry as the chains call it: layer-major tensors, stride_l = B
                import torch
                dev = torch.device("cuda", engine.device)
                jf._register()
                t = [torch.as_tensor(a, device=dev) for a in (nlay, h, vp, vs, rho, noise)]
                logL = torch.zeros(B70, dtype=torch.float64, device=dev)
                misf = torch.zeros((B70, 3), dtype=torch.float64, device=dev)
                err = torch.zeros(B70, dtype=torch.int32, device=dev)
                ymod = torch.zeros((B70, 2 * X7.size), dtype=torch.float64, device=dev)
                torch.cuda.synchronize(dev)
                engine.evaluate_batch_dev(B70, 13, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                                          B70, 1, t[5].data_ptr(), logL.data_ptr(), misf.data_ptr(), err.data_ptr(), ymod=ymod.data_ptr())
                engine.synchronize()
                assert_same((logL.cpu().numpy(), misf.cpu().numpy(), err.cpu().numpy(), ymod.cpu().numpy()), ref, "device entry")


# ---- 6: the same with the shared search switched off by construction; the transforms ----------------------------------------------
PRIVATE = {
    "alone": None,
    "love": lambda: [phase(X7, cls=bh.LoveDispersionPhase)],
    "other periods": lambda: [phase(X7_OTHER)],
    "receiver function": lambda: [prf()],
}


@pytest.mark.parametrize("case", sorted(PRIVATE))
def test_private_search_gives_the_existing_routes_results(engine, case):
    nlay, h, vp, vs, rho = MODELS70
    jf, j0 = pair(engine, PRIVATE[case], first=case != "receiver function")
    noise = noise_for(jf, B70)
    off = jf.targets.index([t for t in jf.targets if isinstance(t, bh.RayleighEllipticity)][0])
    lo = int(sum(np.size(t.obsdata.x) for t in jf.targets[:off]))
    for name, exact, ctx in both_searches(engine):
        with ctx[0], ctx[1], ctx[2]:
            ref = j0.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True)
            got = jf.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True)
            ok = assert_same(got, ref, "%s %s" % (case, name), exact, slice(lo, lo + X7.size))
            assert not ok[NOROOT] and not ok[WATER] and ok[SEDIMENT] and ok.sum() >= B70 - 8   # (a half-space has no Love wave)


@pytest.mark.parametrize("params", [dict(signed=True), dict(ratio="zh"), dict(nsteps=0), dict(signed=True, ratio="zh", nsteps=1)])
@pytest.mark.parametrize("beside", ["shared", "alone"])
def test_transforms_give_the_plugins_bits(engine, params, beside):
    x = np.array([1.0, 2.0, 4.0, 8.0])
    models = [named("sediment"), named("crust"), named("lvz")]
    bad = [a.copy() for a in named("sediment")]
    bad[1][1] = 200.0
    nlay, h, vp, vs, rho = bh.pack_models(models + [tuple(bad)])
    jf, j0 = pair(engine, (lambda: [phase(x)]) if beside == "shared" else None, x=x, **params)
    noise = noise_for(jf, 4)
    ref = j0.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True)
    got = jf.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True)
    assert_same(got, ref, str(params))
    assert list(got[2]) == [0, 0, 0, 1]
    _, y, err = j0.targets[-1].moddata.plugin.run_models(nlay, h, vp, vs, rho)      # SurfEllip.run_models with the same parameters
    assert np.array_equal(bits(got[3][:3, -x.size:]), bits(y[:3])) and list(err) == [0, 0, 0, 1]
    if params.get("signed"):
        assert got[3][0, -x.size + 1] < 0 and np.all(got[3][0, [-4, -2, -1]] > 0)   # the sediment model is prograde at T = 2 s


# ---- 7: one search, not two -------------------------------------------------------------------------------------------------------
def test_shared_search_makes_the_dispersion_launches_of_the_phase_target_alone(engine):
    nlay, h, vp, vs, rho = MODELS70
    alone = bh.JointTarget([phase()], engine=engine)
    shared = bh.JointTarget([phase(), ellip(X7, True)], engine=engine)
    private = bh.JointTarget([phase(X7_OTHER), ellip(X7, True)], engine=engine)
    engine.set_instrumentation(counting=True)
    try:
        out = {}
        for name, jt in (("alone", alone), ("shared", shared), ("private", private)):
            jt.evaluate_batch(nlay, h, vp, vs, noise_for(jt, B70), rho=rho)
            engine.synchronize()
            out[name] = (engine.last_swd_launches(), engine.last_neval())
    finally:
        engine.set_instrumentation()
    print("secular evaluations of the dispersion launches: %r" % {k: v[1] for k, v in out.items()})
    assert out["shared"][0] == out["alone"][0] and out["shared"][1] == out["alone"][1] > 0
    assert out["private"][1] > 1.5 * out["alone"][1]      # a second search's evaluations, where one does not suffice


# ---- 8: repeat calls at a changing batch size --------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["shared", "private"])
def test_failure_rows_are_rewritten_in_full(engine, variant):
    """B = 70, 33, 70 on one registration: the failures of the first call (models 5 and 36) must not survive into the second, whose
    model 5 is another one, nor the second's into the third"""
    nlay, h, vp, vs, rho = MODELS70
    jf = bh.JointTarget([phase(X7 if variant == "shared" else X7_OTHER), ellip(X7, True)], engine=engine)
    noise = noise_for(jf, B70)
    first = jf.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True)
    sel = np.flatnonzero(first[2] == 0)[-33:]            # 33 models that do not fail, where the two that do were
    assert sel[NOROOT] != NOROOT
    mid = jf.evaluate_batch(nlay[sel], *[np.ascontiguousarray(a[:, sel]) for a in (h, vp, vs)], noise[:33],
                            rho=np.ascontiguousarray(rho[:, sel]), want_ymod=True)
    third = jf.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True)
    assert not mid[2].any() and list(np.flatnonzero(first[2])) == [NOROOT, WATER]
    for k in range(3):
        assert np.array_equal(bits(mid[k]), bits(first[k][sel])), k
    ok = first[2] == 0
    assert np.array_equal(bits(mid[3]), bits(first[3][sel]))
    for k in range(3):
        assert np.array_equal(bits(first[k]), bits(third[k])), k
    assert np.array_equal(bits(first[3][ok]), bits(third[3][ok]))


# ---- 9: the host chains -----------------------------------------------------------------------------------------------------------
XC = np.array([2.0, 4.0, 8.0, 12.0, 20.0, 30.0])
PRIORS = {"vs": (2.0, 5.0), "z": (0, 60), "layers": (1, 6), "vpvs": 1.73, "swdnoise_corr": 0.0, "swdnoise_sigma": (1e-3, 0.1),
          "ellnoise_corr": 0.0, "ellnoise_sigma": (1e-3, 0.2)}
INIT = {"iter_burnin": 100, "iter_main": 100, "propdist": (0.025, 0.025, 0.015, 0.005, 0.005), "acceptance": (40, 45)}


@pytest.fixture(scope="module")
def observed(engine):
    m = named("crust")
    with engine.searching("reference"), engine.computing("exact"):
        yd = bh.SurfDisp(XC, "rdispph", engine=engine).run_model(*m)[1]
        ye = bh.SurfEllip(XC, engine=engine).run_model(*m)[1]
    return yd, ye


def chain_targets(observed, fused, s=0, x=XC):
    """site s of an array: the crust model's curves, shifted a little per site; x: the periods of the dispersion curve"""
    yd, ye = observed
    td = bh.RayleighDispersionPhase(x, np.interp(x, XC, yd) * (1.0 + 0.004 * s))
    te = bh.RayleighEllipticity(XC, ye * (1.0 - 0.01 * s), fused=fused)
    return [td, te]


def test_chain_batch_walks_the_existing_routes_run(engine, observed):
    runs = [bh.ChainBatch(bh.JointTarget(chain_targets(observed, fused), engine=engine), [11, 12, 13, 14], INIT, PRIORS,
                          search="reference").run() for fused in (True, False)]
    for a, b in zip(runs[0].chains, runs[1].chains):
        assert np.array_equal(bits(a.likes), bits(b.likes)) and np.array_equal(bits(a.misfits), bits(b.misfits))
        assert np.array_equal(bits(a.currentmodel), bits(b.currentmodel)) and np.array_equal(bits(a.currentnoise), bits(b.currentnoise))
        assert a.accepted.sum() > 0 and np.all(np.asarray(a.likes, dtype=float) > -1e14)


# ---- 10: the device chains --------------------------------------------------------------------------------------------------------
DINIT = dict(INIT, iter_burnin=64, iter_main=64, maxmodels=16)


def test_device_chains_states_are_the_existing_routes_evaluations(engine, observed):
    dc = DeviceChains(chain_targets(observed, True), 8, DINIT, PRIORS, seed=5, search="reference", arith="exact").run()
    st = dc.state_host()
    models = [np.concatenate((st["vs"][:n, c], st["z"][:n, c])) for c, n in enumerate(st["n"])]
    nlay, h, vp, vs = Model.pack_batch(models, st["vpvs"], mantle=None)
    ref = bh.JointTarget(chain_targets(observed, False), engine=engine)
    for t, t0 in zip(ref.targets, dc.targets.targets):
        t.set_noise_law(t0.law())
    with engine.searching("reference"), engine.computing("exact"):
        logL, misfits, err = ref.evaluate_batch(nlay, h, vp, vs, np.ascontiguousarray(st["noise"].T))
    assert not err.any()
    assert np.array_equal(bits(st["like"]), bits(logL)) and np.array_equal(bits(st["misfits"].T), bits(misfits))
    assert (st["accepted"].sum(axis=0) > 0).all()


def test_device_chains_defaults_windows_and_device_record(engine, observed):
    def run(**kw):
        dc = DeviceChains(chain_targets(observed, True), 8, DINIT, PRIORS, seed=5, **kw).run()
        return dc, dc.samples("p1"), dc.samples("p2")

    d1, a1, a2 = run(spec_depth=1)
    for kw in (dict(spec_depth=3), dict(spec_depth=3, record="device")):
        _, b1, b2 = run(**kw)
        for a, b in ((a1, b1), (a2, b2)):
            assert set(a) == set(b)
            for k in a:
                assert np.array_equal(a[k], b[k], equal_nan=True), (kw, k)
    st = d1.state_host()
    assert np.all(np.isfinite(st["like"])) and np.all(st["like"] > -1e14) and np.all(a2["likes"] > -1e14)
    assert (st["accepted"].sum(axis=0) > 0).all()


def test_device_chains_tempered_ladders_run(engine, observed):
    nl, nr = 2, 4
    ladder = np.repeat(np.arange(nl), nr)
    betas = np.tile(1.0 / np.geomspace(1.0, 8.0, nr), nl)
    dc = DeviceChains(chain_targets(observed, True), nl * nr, DINIT, PRIORS, seed=9, betas=betas, ladder=ladder, swap_every=2).run()
    s = dc.samples("p2", cold_only=True)
    assert s["likes"].shape[1] == nl and np.all(np.isfinite(s["likes"])) and np.all(s["likes"] > -1e14)
    assert dc.sweep == 128 // 2


# ---- 11: many stations ------------------------------------------------------------------------------------------------------------
SITE_X = (np.array([2.5, 5.0, 9.0, 14.0, 22.0, 28.0, 30.0]), np.array([3.0, 6.0, 10.0, 18.0]), np.array([2.0, 4.5, 8.0, 12.5, 25.0]))


@pytest.mark.parametrize("per_site_x", [False, True])
def test_site_chains_walk_the_one_site_runs(engine, observed, per_site_x):
    """per_site_x: the dispersion slots at three period sets of 7, 4 and 5, none of them the ellipticity's -- which runs its own
    search in the one-site runs and, under the table of periods, in the run of the three sites"""
    S, Cn = 3, 4
    xs = SITE_X if per_site_x else (XC,) * S
    sites = bh.SiteTargets([bh.JointTarget(chain_targets(observed, True, s, xs[s]), engine=engine) for s in range(S)], per_site_x=per_site_x)
    dc = DeviceChains(sites, Cn, DINIT, PRIORS, seed=21).run()
    for s in range(S):
        one = DeviceChains(chain_targets(observed, True, s, xs[s]), Cn, DINIT, PRIORS, seed=21, chain_offset=s * Cn).run()
        for ph in ("p1", "p2"):
            a, b = dc.samples(ph, site=s), one.samples(ph)
            assert set(a) == set(b)
            for k in a:
                assert np.array_equal(a[k], b[k], equal_nan=True), "site %d %s: %s" % (s, ph, k)
        assert (one.state_host()["accepted"].sum(axis=0) > 0).all()


# ---- 12: argument errors ----------------------------------------------------------------------------------------------------------
def test_targets_set_ellip_argument_errors_change_nothing(engine):
    nlay, h, vp, vs, rho = MODELS70
    jf = bh.JointTarget([phase(), ellip(X7, True)], engine=engine)
    noise = noise_for(jf, B70)
    before = jf.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True)
    L, hd = engine._L, engine._h
    x = np.ascontiguousarray(X7)
    p = C.c_void_p(x.ctypes.data)

    def refused(match, t=1, K=7, per=p, nsteps=2):
        rc = L.bh_targets_set_ellip(hd, t, K, per, nsteps, 0, 0)
        assert rc == -1 and match in L.bh_engine_last_error(hd).decode(), (match, rc, L.bh_engine_last_error(hd))

    refused("no such target", t=2)
    refused("no such target", t=-1)
    refused("not a BH_TARGET_USER", t=0)                 # a dispersion target
    refused("not a BH_TARGET_USER", t=1)                 # the ellipticity itself: its kind is BH_TARGET_ELLIP already
    engine.set_targets([t.engine_desc() for t in (phase(), ellip(X7, False))])   # ... so once more, with a USER target in place
    engine._owner = None
    refused("K differs", K=6)
    long = np.linspace(1.0, 40.0, 61)
    engine.set_targets([dict(ellip(X7, False).engine_desc(), n=61, yobs=np.ones(61))])
    refused("K must be 1..60", t=0, K=61, per=C.c_void_p(long.ctypes.data))
    engine.set_targets([t.engine_desc() for t in (phase(), ellip(X7, False))])
    refused("null periods", per=None)
    for v in (0.0, -1.0, np.nan, np.inf):
        badx = x.copy()
        badx[4] = v
        refused("not finite and positive", per=C.c_void_p(badx.ctypes.data))
    refused("nsteps must be 0..3", nsteps=4)
    refused("nsteps must be 0..3", nsteps=-1)
    with pytest.raises(bh.EngineError, match="no forward model"):    # every refusal left the target a USER target
        engine.evaluate_batch(nlay, h, vp, vs, noise, rho=rho)
    engine.set_sites(np.zeros((2, 14)))
    refused("a site table is in force")
    # a valid set afterwards gives what it gave before
    after = jf.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True)
    ok = before[2] == 0
    for k in range(3):
        assert np.array_equal(bits(before[k]), bits(after[k])), k
    assert np.array_equal(bits(before[3][ok]), bits(after[3][ok]))
    # bh_loglike_batch serves the set as it serves a USER target
    ll = engine.loglike_batch(after[3], noise, np.array([after[2], after[2]]))
    assert np.array_equal(bits(ll[0]), bits(after[0])) and np.array_equal(ll[2], after[2])
