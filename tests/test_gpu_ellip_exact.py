"""Every route to the Rayleigh ellipticity on the GPU against a 110-digit reference on models of the kind a chain proposes
(tests/golden/ellip_exact.npz; tests/ellip_exact.py, tests/golden/gen_ellip_golden.py), and the kernel's edges that no bitwise test
reached, against the restatement (tests/ellip_ref.py).  This file reads the recorded set and ellip_ref only.

The two properties, on every pair with an exact value hv* of every model the route does not fail (G = BH_ELLIP_MISMATCH_MAX):
    safety        |atan(hv) - atan(hv*)| <= G.  In the angle an H/V peak and a zero crossing are as well conditioned as any other
                  value; for hv* between the two expressions of hv it follows from the gate: the angle between them is at most
                  |hv - hv_alt| / (1 + hv^2) <= mismatch <= G where they have one sign.
    certificate   |hv - hv*| <= mismatch |hv| + 1e-12 |hv|: hv* lies between the two expressions.  1e-12 is the rounding floor of
                  the two float64 ratios (<= 2.4e-14 on well-behaved stacks, tests/test_ellip_ref.py).
Before the gate on the mismatch the safety tests fail: 80 of the 437 entries that the call accepted after two polish steps are off
by more than G, the worst by 1.63 rad (tests/test_ellip_exact.py shows it on the CPU).

The properties are per model, as the routes fail: one accepted pair of the set, taken alone, misses the certificate unpolished by
2 % (model 29 at 15 s, both expressions on one side of hv*; tests/test_ellip_exact.py states it) -- another period of its model
meets the gate, so no route hands it out."""
import numpy as np
import pytest

import bayhunter_amd as bh
import ellip_ref as R
from bayhunter_amd import engine as E
from conftest import golden
from test_gpu_ellip_fused import ellip, phase

pytestmark = pytest.mark.gpu

G = R.MISMATCH_MAX
MODEL_ARRAYS = ("h", "vp", "vs", "rho")


@pytest.fixture(scope="module")
def gold():
    g = dict(golden("ellip_exact.npz"))
    g["ok"] = g["noexact"] == 0
    assert G == E.ELLIP_MISMATCH_MAX and g["c"].shape == (71, 8) and g["ok"].sum() >= 250
    return g


def models(g):
    return g["nlay"], g["h"], g["vp"], g["vs"], g["rho"]


def failed_models(g, nsteps, cols=slice(None)):
    """what a route that starts from the oracle's velocities must fail: the search's failure, the polish's flag, the gate"""
    return (g["err"] != 0) | (g["flag%d" % nsteps][:, cols] != 0).any(axis=1)


def angle(hv, hvstar):
    return np.abs(np.arctan(hv) - np.arctan(hvstar))


def pairs_of(g, failed, pairs=None):
    ok = g["ok"] & ~np.asarray(failed, dtype=bool)[:, None]
    return ok if pairs is None else ok & pairs


def assert_safe(g, hv, failed, what, pairs=None, least=200):
    ok = pairs_of(g, failed, pairs)
    ang = angle(hv, g["hvstar"][:, :hv.shape[1]])
    print("%s: %d pairs of %d unfailed models, worst |atan hv - atan hv*| = %.2e" % (what, ok.sum(), (~np.asarray(failed, dtype=bool)).sum(),
                                                                                   ang[ok].max()))
    assert ok.sum() >= least, what
    assert np.all(ang[ok] <= G), what


def assert_certified(g, hv, mis, failed, what, pairs=None, least=200):
    ok = pairs_of(g, failed, pairs)
    err = np.abs(hv - g["hvstar"][:, :hv.shape[1]])
    with np.errstate(invalid="ignore", divide="ignore"):   # (a failed model's entries may be no numbers; they are not looked at)
        bound = mis * np.abs(hv) + 1e-12 * np.abs(hv)
        print("%s: %d pairs, worst |hv - hv*| / (mismatch |hv| + 1e-12 |hv|) = %.3f" % (what, ok.sum(), np.max((err / bound)[ok])))
    assert ok.sum() >= least, what
    assert np.all(err[ok] <= bound[ok]), what


# ---- 1: the velocities handed in ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handed(engine, gold):
    g = gold
    out = {}
    for layout in ("layer_major", "model_major"):
        arrs = [g[k] if layout == "layer_major" else np.ascontiguousarray(g[k].T) for k in MODEL_ARRAYS]
        for nsteps in (0, 2):
            out[nsteps, layout] = engine.swd_ellip(g["nlay"], *arrs, g["periods"], vel=g["c"], err=g["err"], nsteps=nsteps, layout=layout)
    return out


HANDED = pytest.mark.parametrize("nsteps,layout", [(n, lay) for n in (0, 2) for lay in ("layer_major", "model_major")])


@HANDED
def test_handed_in_velocities_give_the_stored_restatement(gold, handed, nsteps, layout):
    g, o = gold, handed[nsteps, layout]
    assert R.same_bits(o["hv"], g["hv%d" % nsteps]) and R.same_bits(o["mismatch"], g["mis%d" % nsteps])
    assert R.same_bits(o["c"], g["cpol%d" % nsteps])
    assert np.array_equal(o["flag"] != 0, (g["flag%d" % nsteps] != 0).any(axis=1))
    assert o["flag"][69] == 1 and np.isnan(o["hv"][69]).all()                       # under water
    assert o["flag"][70] == 0 and not o["hv"][70].any() and not o["c"][70].any()    # the search failed: a zero row, no flag


@HANDED
def test_handed_in_safety(gold, handed, nsteps, layout):
    o = handed[nsteps, layout]
    failed = (o["err"] != 0) | (o["flag"] != 0)
    assert np.array_equal(failed, failed_models(gold, nsteps))
    assert_safe(gold, o["hv"], failed, "handed in, %d steps, %s" % (nsteps, layout))


@HANDED
def test_handed_in_certificate(gold, handed, nsteps, layout):
    o = handed[nsteps, layout]
    assert_certified(gold, o["hv"], o["mismatch"], (o["err"] != 0) | (o["flag"] != 0), "handed in, %d steps, %s" % (nsteps, layout))


# ---- 2: behind the engine's own search ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("search,arith", [("fast", "fast"), ("reference", "exact")])
def test_own_search(engine, gold, search, arith):
    g = gold
    with engine.searching(search), engine.computing(arith):
        o = engine.swd_ellip(*models(g), g["periods"])
    found = (o["err"] == 0)[:, None] & (g["c"] > 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        near = found & (np.abs(o["vel"] / g["c"] - 1.0) <= 2e-6)
    share = near.sum() / float(found.sum())
    print("%s search: %d of %d velocities within 2e-6 of the oracle's (%.1f %%); err on models %s"
          % (search, near.sum(), found.sum(), 100.0 * share, list(np.flatnonzero(o["err"]))))
    assert found.sum() >= 500 and share >= 0.95
    if search == "reference":   # the oracle's bits: the same failures and the stored restatement
        assert near.sum() == found.sum() and np.array_equal(o["vel"], g["c"]) and np.array_equal(o["err"], g["err"])
        assert R.same_bits(o["hv"], g["hv2"]) and np.array_equal(o["flag"] != 0, (g["flag2"] != 0).any(axis=1))
    failed = (o["err"] != 0) | (o["flag"] != 0)
    assert_safe(g, o["hv"], failed, "own %s search" % search, near, least=150)
    assert_certified(g, o["hv"], o["mismatch"], failed, "own %s search" % search, near, least=150)


# ---- 3: the fused call, the plugin -------------------------------------------------------------------------------------------------
FUSED = {"shared": (True, {}), "alone": (False, {}), "signed": (True, dict(signed=True)), "zh": (True, dict(ratio="zh"))}


def undo(y, params):
    """hv (or |hv|) from the target's columns"""
    with np.errstate(divide="ignore"):
        return 1.0 / y if params.get("ratio") == "zh" else y


def fused_call(engine, g, beside, params):
    """set_targets, set_target_ellip, evaluate_batch: a USER target given the forward model, beside a Rayleigh phase target at the
    same periods (one search) or alone (its own)"""
    x = g["periods"]
    user = ellip(x, False).engine_desc()
    assert user["kind"] == E.TARGET_USER and "nsteps" not in user
    descs = ([phase(x).engine_desc()] if beside else []) + [user]
    engine.set_targets(descs)
    engine._owner = None
    engine.set_target_ellip(len(descs) - 1, x, nsteps=2, signed=params.get("signed", False), ratio=params.get("ratio", "hv"))
    B = g["nlay"].size
    noise = np.tile(np.array([0.0, 0.05] * len(descs)), (B, 1))
    nlay, h, vp, vs, rho = models(g)
    return engine.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True)


@pytest.mark.parametrize("case", sorted(FUSED))
def test_fused_call(engine, gold, case):
    g = gold
    beside, params = FUSED[case]
    K = g["periods"].size
    logL, misfits, err, ymod = fused_call(engine, g, beside, params)
    want = failed_models(g, 2)
    assert np.array_equal(err != 0, want), "failed %s, expected %s" % (np.flatnonzero(err), np.flatnonzero(want))
    assert want.sum() >= 30 and want[69] and want[70] and not want[66]              # (the gate fails half the prior-drawn models)
    assert np.all(logL[want] == -1e15) and np.all(misfits[want] == 1e15) and np.all(np.isfinite(logL[~want]))
    y = ymod[:, -K:]
    if beside:
        assert np.array_equal(ymod[~want, :K], g["c"][~want])                       # the one search is the oracle's
    hv2 = g["hv2"] if params.get("signed") else np.abs(g["hv2"])
    assert R.same_bits(y[~want], undo(hv2, params)[~want])                          # bh_swd_ellip's bits, transformed
    hv = undo(y, params)
    star = dict(g, hvstar=g["hvstar"] if params.get("signed") else np.abs(g["hvstar"]))
    assert_safe(star, hv, want, "fused %s" % case)
    assert_certified(star, hv, g["mis2"], want, "fused %s" % case)


def test_run_models_fails_the_models_the_fused_call_fails(engine, gold):
    g = gold
    nlay, h, vp, vs, rho = models(g)
    _, y, err = bh.SurfEllip(g["periods"], engine=engine).run_models(nlay, h, vp, vs, rho)
    fused = fused_call(engine, g, True, {})
    assert np.array_equal(err != 0, fused[2] != 0) and np.array_equal(err != 0, failed_models(g, 2))
    assert np.isnan(y[err != 0]).all() and R.same_bits(y[err == 0], fused[3][err == 0][:, -g["periods"].size:])
    assert_safe(dict(g, hvstar=np.abs(g["hvstar"])), np.nan_to_num(y), err != 0, "SurfEllip.run_models")


def test_site_build(engine, gold):
    """two sites over the same 71 models: all eight periods, and the first three (the search visits the periods in order, so
    its velocities at the first three are those of the full set); the ellipticity beside the phase velocities at each site's own"""
    g = gold
    B, K = g["c"].shape
    xs = (g["periods"], g["periods"][:3])
    st = bh.SiteTargets([[phase(x), ellip(x, True)] for x in xs], engine=engine, per_site_x="all", missing=True, per_site_ellip=True)
    nlay, h, vp, vs, rho = [np.concatenate([a, a], axis=-1) for a in models(g)]
    site = np.repeat(np.arange(2, dtype=np.int32), B)
    noise = np.tile(np.array([0.0, 0.05, 0.0, 0.07]), (2 * B, 1))
    logL, misfits, err, ymod = st.evaluate_batch(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
    assert ymod.shape == (2 * B, 2 * K)
    for s, n in enumerate((K, 3)):
        rows = slice(s * B, (s + 1) * B)
        vel, y, e = ymod[rows, :n], ymod[rows, K:K + n], err[rows] != 0
        if s == 0:
            want, hv2 = failed_models(g, 2), g["hv2"]
        else:   # (the model whose search fails from 15 s on has its first three velocities: the restatement says what becomes of them)
            ref = R.ellip_batch(g["nlay"], g["h"], g["vp"], g["vs"], g["rho"], xs[1], vel, np.zeros(B, dtype=np.int32), 2)
            want, hv2 = ref[3] != 0, ref[0]
            live = np.arange(B) != 70
            assert np.array_equal(want[live], failed_models(g, 2, slice(0, 3))[live]) and R.same_bits(hv2[live], g["hv2"][live, :3])
            assert not want[70] and np.all(hv2[70] > 0)
        assert np.array_equal(e, want), "site %d: failed %s, expected %s" % (s, np.flatnonzero(e), np.flatnonzero(want))
        assert np.array_equal(vel[~want], g["c"][~want, :n]) and np.all(logL[rows][want] == -1e15)
        assert R.same_bits(y[~want], np.abs(hv2[~want, :n]))
        assert np.all(ymod[rows, n:K].view(np.int64) == 0) and np.all(ymod[rows, K + n:].view(np.int64) == 0)   # beyond the site's count
        star = dict(g, ok=g["ok"][:, :n], hvstar=np.abs(g["hvstar"]))
        assert_safe(star, y, want, "site %d" % s, least=200 if s == 0 else 80)
        assert_certified(star, y, g["mis2"][:, :n], want, "site %d" % s, least=200 if s == 0 else 80)


# ---- 4: edges of the kernel, against the restatement ------------------------------------------------------------------------------
def dev_ellip(engine, Lmax, nlay, arrays, sl, sb, periods, vel, err, nsteps):
    """swd_ellip_dev on torch tensors as they are (any strides the caller says) -> hv, mismatch, cpol, flag"""
    import torch
    dev = torch.device("cuda", engine.device)
    B, K = vel.shape
    t = [torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in
         (np.asarray(nlay, dtype=np.int32),) + tuple(arrays) + (np.asarray(periods, dtype=float), vel, np.asarray(err, dtype=np.int32))]
    out = [torch.full((B, K), 7.0, dtype=torch.float64, device=dev) for _ in range(3)]
    flag = torch.full((B,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    engine.swd_ellip_dev(B, Lmax, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), sl, sb, K,
                         t[5].data_ptr(), t[6].data_ptr(), t[7].data_ptr(), out[0].data_ptr(), flag.data_ptr(), have_vel=True,
                         nsteps=nsteps, mismatch=out[1].data_ptr(), cpol=out[2].data_ptr())
    engine.synchronize()
    return [o.cpu().numpy() for o in out] + [flag.cpu().numpy()]


def assert_bits(got, ref, what):
    for name, a, b in zip(("hv", "mismatch", "cpol"), got, ref):
        assert R.same_bits(a, b), "%s: %s" % (what, name)
    assert np.array_equal(got[3], ref[3]), "%s: flag" % what


@pytest.mark.parametrize("nsteps", [1, 3])
def test_one_and_three_polish_steps(engine, gold, nsteps):
    g = gold
    sel = np.r_[0:24, 48:56, 64:71]                     # prior-drawn, sorted ones, the named ones
    nlay, arrs = g["nlay"][sel], [np.ascontiguousarray(g[k][:, sel]) for k in MODEL_ARRAYS]
    vel, err = np.ascontiguousarray(g["c"][sel]), g["err"][sel]
    ref = R.ellip_batch(nlay, *arrs, g["periods"], vel, err, nsteps)
    o = engine.swd_ellip(nlay, *arrs, g["periods"], vel=vel, err=err, nsteps=nsteps)
    assert_bits((o["hv"], o["mismatch"], o["c"], o["flag"]), ref, "%d steps" % nsteps)
    assert ref[3].sum() >= 10 and (ref[3] == 0).sum() >= 10


def test_rows_without_layers_and_with_too_many_are_zero_rows(engine, gold):
    g = gold
    sel = np.arange(60, 68)
    nlay = g["nlay"][sel].copy()
    nlay[[1, 5]] = 0, 13                                 # Lmax = 12
    arrs = [np.ascontiguousarray(g[k][:, sel]) for k in MODEL_ARRAYS]
    vel, err = np.ascontiguousarray(g["c"][sel]), np.zeros(sel.size, dtype=np.int32)
    ref = R.ellip_batch(nlay, *arrs, g["periods"], vel, err, 2)
    got = dev_ellip(engine, 12, nlay, arrs, sel.size, 1, g["periods"], vel, err, 2)
    assert_bits(got, ref, "nlay 0 and Lmax + 1")
    for b in (1, 5):
        assert all(np.all(a[b].view(np.int64) == 0) for a in got[:3]) and got[3][b] == 0
    assert np.any(got[0][[0, 2, 3, 4, 6, 7]] != 0)


def test_a_hundred_layers_beside_two_in_one_wavefront(engine):
    """Lmax = 100: a gradient of 99 layers of 0.4 km over its half-space between two-layer models; 3 models x 4 periods = 12 lanes"""
    n = 100
    vs = 2.6 + (4.5 - 2.6) * np.arange(n) / (n - 1)
    deep = (np.r_[np.full(n - 1, 0.4), 0.0], vs * 1.75, vs, vs * 1.75 * 0.32 + 0.77)
    two = [(np.array([h, 0.0]), np.array([5.2, 7.9]), np.array([3.0, 4.5]), np.array([2.4, 3.3])) for h in (3.0, 11.0)]
    mods = [two[0], deep, two[1]]
    periods = [2.0, 6.0, 14.0, 30.0]
    nlay, h, vp, vs_, rho = bh.pack_models(mods)
    assert h.shape == (100, 3) and list(nlay) == [2, 100, 2]
    deltas = (2.0e-6, -1.0e-6, 0.0, 5.0e-7)
    vel = np.array([[c * (1.0 + deltas[(b + k) % 4]) for k, c in enumerate(R.fundamental_roots(R.round_model(*m), periods))]
                    for b, m in enumerate(mods)])
    err = np.zeros(3, dtype=np.int32)
    for nsteps in (0, 2):
        ref = R.ellip_batch(nlay, h, vp, vs_, rho, periods, vel, err, nsteps)
        o = engine.swd_ellip(nlay, h, vp, vs_, rho, periods, vel=vel, err=err, nsteps=nsteps)
        assert_bits((o["hv"], o["mismatch"], o["c"], o["flag"]), ref, "100 layers, %d steps" % nsteps)
        assert not ref[3].any() and np.all(ref[0] > 0.3) and (nsteps == 0 or np.all(ref[1] <= 1e-11))


@pytest.mark.parametrize("layout", ["layer_major", "model_major"])
def test_device_entry_with_padded_strides(engine, gold, layout):
    """sl and sb that are not the packed ones; the padding holds NaN"""
    g = gold
    sel = np.r_[40:52, 64:71]
    B, L = sel.size, 12
    nlay, vel, err = g["nlay"][sel], np.ascontiguousarray(g["c"][sel]), g["err"][sel]
    packed = [np.ascontiguousarray(g[k][:, sel]) for k in MODEL_ARRAYS]
    ref = R.ellip_batch(nlay, *packed, g["periods"], vel, err, 2)
    if layout == "layer_major":
        sl, sb = B + 5, 1
        padded = [np.full((L, sl), np.nan) for _ in packed]
        for p, a in zip(padded, packed):
            p[:, :B] = a
    else:
        sl, sb = 1, L + 3
        padded = [np.full((B, sb), np.nan) for _ in packed]
        for p, a in zip(padded, packed):
            p[:, :L] = a.T
    assert_bits(dev_ellip(engine, L, nlay, padded, sl, sb, g["periods"], vel, err, 2), ref, "padded %s" % layout)
    assert np.array_equal(ref[3] != 0, failed_models(g, 2)[sel] & (err == 0))


def test_two_workgroups_of_ragged_wavefronts(engine, gold):
    """B = 70, K = 7: 490 lanes, two workgroups; 64 / 7 is no integer, so models straddle wavefronts, and model 36 the workgroups;
    the layer counts of 2 .. 12 make every wavefront's loop bound another"""
    g = gold
    nlay, arrs = g["nlay"][:70], [np.ascontiguousarray(g[k][:, :70]) for k in MODEL_ARRAYS]
    periods = g["periods"][1:]
    vel, err = np.ascontiguousarray(g["c"][:70, 1:]), g["err"][:70]
    assert vel.shape == (70, 7) and len(set(nlay[:9])) > 3
    ref = R.ellip_batch(nlay, *arrs, periods, vel, err, 2)
    for layout in ("layer_major", "model_major"):
        a = arrs if layout == "layer_major" else [np.ascontiguousarray(x.T) for x in arrs]
        o = engine.swd_ellip(nlay, *a, periods, vel=vel, err=err, nsteps=2, layout=layout)
        assert_bits((o["hv"], o["mismatch"], o["c"], o["flag"]), ref, "70 x 7 %s" % layout)
    assert R.same_bits(ref[0], g["hv2"][:70, 1:]) and np.array_equal(ref[3] != 0, (g["flag2"][:70, 1:] != 0).any(axis=1))
