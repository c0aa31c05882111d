"""Sites that lack some of the array's targets, on the MI355X (include/bh_engine_sites_missing.h, SiteTargets(missing=True)).
The rule under test: a model of site s gets the logL, misfits, err and synthetics of a one-site bh_evaluate_batch whose descriptors
are the targets site s HAS; a slot it lacks adds nothing, has misfit 0, zero columns and never sets err.  And a site of a
DeviceChains walks the chain of its one-site DeviceChains over the targets it has.  tests/test_sites_missing_host.py asserts with
the oracle that the batches used here are not about failed rows."""
import os

import numpy as np
import pytest

from conftest import golden
import bayhunter_amd as bh
from bayhunter_amd import engine as E
from bayhunter_amd.device_chains import DeviceChains
from bayhunter_amd.sites import slot_columns
from bayhunter_amd.synth import synth_models
from test_gpu_sites_x import batch, bits, configure, PERIOD_SETS, NSITES, SITE_P, B_MODELS, PRIORS

pytestmark = pytest.mark.gpu

# A slot: ("swd", iwave, igr, mode, law, period scale, shift -- site s has PERIOD_SETS[(s + shift) % NSITES] x scale) or
# ("rf", waveno, law).  A structure: its slots and, per site, which of them the site has.
R_PH = ("swd", 2, 0, 1, E.LAW_NOCORR, 1.0, 0)
L_PH = ("swd", 1, 0, 1, E.LAW_NOCORR_SCALED, 1.0, 1)
L_PH_EXP = ("swd", 1, 0, 1, E.LAW_EXP, 1.0, 1)
R_GR = ("swd", 2, 1, 1, E.LAW_EXP, 1.0, 2)
R_M2 = ("swd", 2, 0, 2, E.LAW_NOCORR, 0.25, 3)
P_RF = ("rf", 0, E.LAW_EXP)
S_RF = ("rf", 1, E.LAW_EXP)
STRUCTURES = {
    # every kind; site 2 has receiver functions only, site 3 dispersion only; every slot is lacked by two sites or more
    "full": ([R_PH, L_PH, R_GR, R_M2, P_RF, S_RF],
             ["111111", "101010", "000011", "111100", "010101", "110010"]),
    # fundamental-mode phase velocities and receiver functions: the trial-per-lane kernel under the engine's defaults
    "phase_rf": ([R_PH, L_PH, P_RF, S_RF], ["1111", "1010", "0011", "1100", "0101", "1110"]),
    # a group velocity beside phase velocities: under the defaults the mixed call takes the group kernel
    "group_mix": ([R_PH, L_PH_EXP, R_GR], ["111", "110", "101", "011", "100", "001"]),
}
NRF = 150


def present_of(name):
    return np.array([[c == "1" for c in row] for row in STRUCTURES[name][1]], dtype=bool)


def slot_periods(spec, s):
    return PERIOD_SETS[(s + spec[6]) % NSITES] * spec[5]


def site_descs_missing(name, rs):
    """per site, per slot: the one-site descriptor, or None where the site lacks the slot (the random numbers are drawn either
    way: a site's data do not depend on what the other sites have)"""
    slots, _ = STRUCTURES[name]
    present = present_of(name)
    out = []
    for s in range(NSITES):
        row = []
        for i, spec in enumerate(slots):
            if spec[0] == "swd":
                per = slot_periods(spec, s)
                d = dict(kind=E.TARGET_SWD, law=spec[4], n=per.size, x=per, iwave=spec[1], igr=spec[2], mode=spec[3],
                         yobs=3.0 + 0.3 * np.log(per / spec[5]) + rs.normal(0, 0.05, per.size))
                yerr = rs.uniform(0.01, 0.05, per.size)
                if spec[4] == E.LAW_NOCORR_SCALED:
                    d["yerr"] = yerr
            else:
                d = dict(kind=E.TARGET_RF, law=spec[2], n=NRF, waveno=spec[1], nsamp=512, p=float(SITE_P[s]), gauss=2.5, fsamp=5.0,
                         tshift=5.0, nsv=0.0, yobs=rs.normal(0, 0.05, NRF))
            row.append(d if present[s, i] else None)
        out.append(row)
    return out


def tables_missing(descs):
    """capacity descriptors of the slots (from the first site that has each; placeholders on dispersion slots) and the tables of
    bh_sites_set_missing -- count 0 and placeholders for an absent (site, slot) -- and of bh_sites_set_rf"""
    S, nt = len(descs), len(descs[0])
    n = np.array([[0 if d is None else d["n"] for d in ds] for ds in descs], dtype=np.int32)
    cap = n.max(axis=0)
    off = np.concatenate([[0], np.cumsum(cap)]).astype(int)
    x, yobs, yerr = np.zeros((S, off[-1])), np.zeros((S, off[-1])), np.ones((S, off[-1]))
    p = np.zeros((S, nt))
    for s, ds in enumerate(descs):
        for t, d in enumerate(ds):
            if d is None:
                continue
            c = slice(off[t], off[t] + d["n"])
            yobs[s, c] = d["yobs"]
            if d["kind"] == E.TARGET_SWD:
                x[s, c] = d["x"]
            if "yerr" in d:
                yerr[s, c] = d["yerr"]
            p[s, t] = d.get("p", 0.0)
    caps = []
    for t in range(nt):
        d = dict(next(ds[t] for ds in descs if ds[t] is not None))
        if d["kind"] == E.TARGET_SWD:
            d.update(n=int(cap[t]), x=np.ones(cap[t]), yobs=np.zeros(cap[t]))
            if "yerr" in d:
                d["yerr"] = np.ones(cap[t])
        caps.append(d)
    scaled = any("yerr" in d for d in caps)
    return caps, n, x, yobs, (yerr if scaled else None), p, np.zeros_like(p), off


def register_missing(eng, descs):
    caps, n, x, yobs, yerr, p, nsv, off = tables_missing(descs)
    eng.set_targets(caps)
    eng.set_sites_missing(n, x, yobs, yerr)
    eng.set_sites_rf(p, nsv)
    return n, off


def noise_slots(name, rs, B):
    slots = STRUCTURES[name][0]
    noise = np.column_stack([rs.uniform(0.1, 0.6, B) if i % 2 == 0 else rs.uniform(0.02, 0.1, B) for i in range(2 * len(slots))])
    for t, spec in enumerate(slots):
        if (spec[4] if spec[0] == "swd" else spec[2]) != E.LAW_EXP:
            noise[:, 2 * t] = 0.0
    return noise


def one_site(eng, ds, mods, noise, present_row):
    """the one-site call of a site: the descriptors it has, its own noise columns"""
    nlay, h, vp, vs, rho = mods
    eng.set_targets([d for d in ds if d is not None])
    return eng.evaluate_batch(nlay, h, vp, vs, noise[:, slot_columns(present_row)[0]], rho=rho, want_ymod=True)


def assert_the_rule(got, ref, m, present_row, ns, off, what):
    """models m of one site: logL, err, the present misfits and the joint one, the present columns of ymod -- failed rows and the
    zeros beyond a site's own periods included -- equal the one-site call bit for bit; absent misfits 0, absent columns zeros"""
    logL, misf, err, ymod = got
    _, mcol = slot_columns(present_row)
    assert np.array_equal(bits(logL[m]), bits(ref[0][m])), what + ": logL"
    assert np.array_equal(err[m], ref[2][m]), what + ": err"
    assert np.array_equal(bits(misf[m][:, mcol]), bits(ref[1][m])), what + ": misfits"
    o = 0
    for t, has in enumerate(present_row):
        cols = ymod[m, off[t]:off[t + 1]]
        if not has:
            assert np.all(misf[m, t] == 0.0), "%s: misfit of absent slot %d" % (what, t)
            assert np.all(bits(cols) == 0), "%s: columns of absent slot %d" % (what, t)
            continue
        k = ns[t]
        assert np.array_equal(bits(cols[:, :k]), bits(ref[3][m, o:o + k])), "%s: ymod of slot %d" % (what, t)
        assert np.all(bits(cols[:, k:]) == 0), "%s: beyond the periods of slot %d" % (what, t)
        o += k
    assert o == ref[3].shape[1]


def eval_device(eng, models, noise, site, ldy):
    """bh_evaluate_sites on device memory with ymod and misfits pre-filled with NaN: a column or a misfit that reads 0 afterwards
    was WRITTEN as 0 by a kernel (tests/test_gpu_sites.py's helper hands in zeroed arrays)"""
    import torch
    nlay, h, vp, vs, rho = models
    L, B = h.shape
    dev = torch.device("cuda", 0)
    T = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)
    tn, th, tvp, tvs, trho = T(nlay, torch.int32), T(h), T(vp), T(vs), T(rho)
    tsite, tnoise = T(site, torch.int32), T(noise)
    nan = float("nan")
    logL = torch.full((B,), nan, dtype=torch.float64, device=dev)
    misf = torch.full((B, len(noise[0]) // 2 + 1), nan, dtype=torch.float64, device=dev)
    err, ymod = torch.full((B,), -7, dtype=torch.int32, device=dev), torch.full((B, ldy), nan, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    eng.evaluate_sites_dev(B, L, tn.data_ptr(), th.data_ptr(), tvp.data_ptr(), tvs.data_ptr(), trho.data_ptr(), B, 1,
                           tsite.data_ptr(), tnoise.data_ptr(), logL.data_ptr(), misf.data_ptr(), err.data_ptr(), ymod.data_ptr())
    eng.synchronize()
    return logL.cpu().numpy(), misf.cpu().numpy(), err.cpu().numpy(), ymod.cpu().numpy()


def small_batch(family, Lmax, B=96):
    nlay, h, vp, vs, rho, site = batch(family, Lmax)
    return nlay[:B], h[:, :B], vp[:, :B], vs[:, :B], rho[:, :B], site[:B]


def big_batch(B=2200):
    rs = np.random.RandomState(700 + B)
    mods = synth_models(rs, B, 12, ragged=True)
    return mods + ((rs.permutation(B) % NSITES).astype(np.int32),)


# the batches of the "reference" test: (name, maker) -- 660 models in arrays of 8 / 21 / 40 layers, 96 of them, 2200 models
REF_BATCHES = [("synth8", lambda: batch("synth", 8)), ("prior21", lambda: batch("prior", 21)), ("synth40", lambda: batch("synth", 40)),
               ("small21", lambda: small_batch("synth", 21)), ("big12", big_batch)]


@pytest.mark.parametrize("which,gsplit", [(b[0], 1 << 24) for b in REF_BATCHES] + [("prior21", 0), ("small21", 0)])
def test_reference_search_every_site_equals_its_one_site_call(engine, which, gsplit):
    """Every kind of slot in one call, some sites lacking each: the rule, bit for bit, with a group velocity's second roots in
    their own launch and in the chain's (swd_gsplit = 0), from host and from device memory."""
    nlay, h, vp, vs, rho, site = dict(REF_BATCHES)[which]()
    mods, B = (nlay, h, vp, vs, rho), nlay.size
    rs = np.random.RandomState(5 + B)
    descs = site_descs_missing("full", rs)
    present = present_of("full")
    noise = noise_slots("full", rs, B)
    configure(engine, "reference", 0)
    assert engine.tuning("swd_gsplit") == 1 << 24
    engine.set_tuning("swd_gsplit", gsplit)
    try:
        refs = [one_site(engine, descs[s], mods, noise, present[s]) for s in range(NSITES)]
        n, off = register_missing(engine, descs)
        got = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
        nsecond = sum(1 for l in engine.last_swd_launches() if l["role"] == "second")
        assert nsecond == (1 if gsplit else 0)
        dev = eval_device(engine, mods, noise, site, engine.ldy)
    finally:
        engine.set_tuning("swd_gsplit", 1 << 24)
    assert got[3].shape == (B, off[-1])
    for s in range(NSITES):
        m = site == s
        assert m.sum() >= 8
        assert_the_rule(got, refs[s], m, present[s], n[s], off, "%s site %d host" % (which, s))
        assert_the_rule(dev, refs[s], m, present[s], n[s], off, "%s site %d device" % (which, s))
    ok = got[2] == 0
    assert 0 < (~ok).sum() < 0.5 * B and np.isfinite(got[0][ok]).all()


def test_skipping_logL_without_synthetics_equals_with(engine):
    """without the synthetics asked for (a sampler's call) the same logL, misfits and err"""
    nlay, h, vp, vs, rho, site = batch("prior", 21)
    rs = np.random.RandomState(11)
    descs = site_descs_missing("full", rs)
    noise = noise_slots("full", rs, B_MODELS)
    configure(engine, "reference", 0)
    register_missing(engine, descs)
    a = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
    b = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho)
    for x, y in zip(a[:3], b):
        assert np.array_equal(bits(x), bits(y))


@pytest.mark.parametrize("trials", [32, 64])
@pytest.mark.parametrize("which", ["synth8", "prior21", "small21"])
def test_defaults_phase_only_slots_take_the_lean_kernel_and_keep_the_bits(engine, which, trials):
    """Fundamental-mode phase velocities and receiver functions under the engine's defaults with the trial count pinned: the
    mixed call and every one-site call take the trial-per-lane kernel, whose result is a function of the model and the trial
    count only -- the rule holds bit for bit."""
    nlay, h, vp, vs, rho, site = dict(REF_BATCHES)[which]()
    mods, B = (nlay, h, vp, vs, rho), nlay.size
    rs = np.random.RandomState(trials + B)
    descs = site_descs_missing("phase_rf", rs)
    present = present_of("phase_rf")
    noise = noise_slots("phase_rf", rs, B)
    try:
        configure(engine, "default", trials)
        refs = []
        for s in range(NSITES):
            refs.append(one_site(engine, descs[s], mods, noise, present[s]))
            if present[s, :2].any():
                assert engine.last_swd_kernel() == "lean"
        n, off = register_missing(engine, descs)
        got = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
        assert engine.last_swd_kernel() == "lean"
        dev = eval_device(engine, mods, noise, site, engine.ldy)
    finally:
        engine.set_swd_trials(0)
    for s in range(NSITES):
        m = site == s
        assert_the_rule(got, refs[s], m, present[s], n[s], off, "%s trials %d site %d host" % (which, trials, s))
        assert_the_rule(dev, refs[s], m, present[s], n[s], off, "%s trials %d site %d device" % (which, trials, s))


@pytest.mark.parametrize("which", ["prior21", "small21"])
def test_defaults_with_a_group_slot(engine, which):
    """A group-velocity slot beside phase-velocity slots under the engine's defaults: the mixed call takes the group kernel, the
    one-site call of a site without the group curve the trial-per-lane kernel.  What holds between those: phase
    velocities within 2e-6 relative, failure flags and zero rows identical, group velocities bit for bit."""
    nlay, h, vp, vs, rho, site = dict(REF_BATCHES)[which]()
    mods, B = (nlay, h, vp, vs, rho), nlay.size
    rs = np.random.RandomState(77 + B)
    descs = site_descs_missing("group_mix", rs)
    present = present_of("group_mix")
    noise = noise_slots("group_mix", rs, B)
    try:
        configure(engine, "default", 32)
        refs, kernels = [], []
        for s in range(NSITES):
            refs.append(one_site(engine, descs[s], mods, noise, present[s]))
            kernels.append(engine.last_swd_kernel())
        n, off = register_missing(engine, descs)
        got = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
        assert engine.last_swd_kernel() == "group" and "lean" in kernels
    finally:
        engine.set_swd_trials(0)
    logL, misf, err, ymod = got
    worst = 0.0
    for s in range(NSITES):
        m = site == s
        ref = refs[s]
        assert np.array_equal(err[m], ref[2][m]), "site %d: failure flags" % s
        o = 0
        for t, has in enumerate(present[s]):
            cols = ymod[m, off[t]:off[t + 1]]
            if not has:
                assert np.all(bits(cols) == 0) and np.all(misf[m, t] == 0.0)
                continue
            k = n[s, t]
            a, b = cols[:, :k], ref[3][m, o:o + k]
            o += k
            assert np.array_equal(a == 0.0, b == 0.0), "site %d slot %d: zero cells" % (s, t)
            assert np.all(bits(cols[:, k:]) == 0)
            if STRUCTURES["group_mix"][0][t][2] == 1:
                assert np.array_equal(bits(a), bits(b)), "site %d: group velocities" % s
            else:
                nz = b != 0.0
                rel = np.abs(a[nz] - b[nz]) / np.abs(b[nz])
                worst = max(worst, float(rel.max()) if rel.size else 0.0)
                print("site %d slot %d: phase velocities within %.3e relative" % (s, t, rel.max() if rel.size else 0.0))
                assert np.all(rel <= 2e-6), "site %d slot %d: %.3e" % (s, t, rel.max())
    print("worst relative difference of a phase velocity: %.3e" % worst)


def test_entry_point_refusals_and_a_site_out_of_range(engine):
    rs = np.random.RandomState(4)
    descs = site_descs_missing("full", rs)
    present = present_of("full")
    nlay, h, vp, vs, rho, site = small_batch("synth", 21, 120)
    mods, B = (nlay, h, vp, vs, rho), 120
    noise = noise_slots("full", rs, B)
    caps, n, x, yobs, yerr, p, nsv, off = tables_missing(descs)
    L, hd = engine._L, engine._h
    P = lambda a: a.ctypes.data

    def rc(entry, n_=n):
        return entry(hd, NSITES, P(np.ascontiguousarray(n_)), P(x), P(yobs), P(yerr))

    configure(engine, "reference", 0)
    engine.set_targets(caps)
    assert rc(L.bh_sites_set_missing) == E.BH_OK
    engine.set_targets(caps)
    for entry in (L.bh_sites_set_x, L.bh_sites_set_x_all):      # the older entry points keep refusing a count below 1
        assert rc(entry) == E.BH_EINVAL
    b = n.copy()
    b[2, :] = 0                                                 # a site with no target
    assert rc(L.bh_sites_set_missing, b) == E.BH_EINVAL and b"site with no target" in L.bh_engine_last_error(hd)
    b = n.copy()
    b[:, 3] = 0                                                 # a slot with no site
    assert rc(L.bh_sites_set_missing, b) == E.BH_EINVAL and b"no site has" in L.bh_engine_last_error(hd)
    b = n.copy()
    b[0, 4] = NRF - 1                                           # a receiver function's count is 0 or its descriptor's
    assert rc(L.bh_sites_set_missing, b) == E.BH_EINVAL
    b = n.copy()
    b[0, 0] = -1
    assert rc(L.bh_sites_set_missing, b) == E.BH_EINVAL
    g = [dict(d) for d in caps]                                 # the Gauss law on a slot that some site lacks
    g[5].update(law=E.LAW_GAUSS, rinv=np.eye(NRF), logdet_r=0.0)
    engine.set_targets(g)
    assert rc(L.bh_sites_set_missing) == E.BH_EUNSUPPORTED
    full = n.copy()
    full[:, 5] = NRF                                            # ... present everywhere it is served
    full[2, 4], full[3, 0] = NRF, 0
    assert rc(L.bh_sites_set_missing, full) == E.BH_OK
    # a receiver-function slot needs the table of bh_sites_set_rf: the coefficient stage finds the model's site there
    engine.set_targets(caps)
    engine.set_sites_missing(n, x, yobs, yerr)
    with pytest.raises(E.EngineError, match="bh_sites_set_rf"):
        engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho)
    engine.set_sites_rf(p, nsv)
    own = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
    wild = site.copy()
    wild[5], wild[17] = NSITES, -1
    keep = np.ones(B, bool)
    keep[[5, 17]] = False
    dev = eval_device(engine, mods, noise, wild, engine.ldy)
    for k in (5, 17):                                           # out of range: fails in band
        assert dev[2][k] == 1 and dev[0][k] == -1e15 and np.all(dev[1][k] == 1e15) and np.all(dev[3][k, :off[4]] == 0.0)
    for a, c in zip(dev, own):
        assert np.array_equal(bits(a[keep]), bits(c[keep]))
    with pytest.raises(E.EngineError, match="out of range"):
        engine.evaluate_sites(nlay, h, vp, vs, noise, wild, rho=rho)
    # a model with absurd values fails the dispersion targets; at a site that has receiver functions only it is theirs alone
    bad_vs = vs.copy()
    rfonly = np.flatnonzero(site == 2)[:3]
    other = np.flatnonzero(site == 0)[:3]
    bad_vs[0, rfonly] = 200.0
    bad_vs[0, other] = 200.0
    got = engine.evaluate_sites(nlay, h, vp, bad_vs, noise, site, rho=rho, want_ymod=True)
    ref = one_site(engine, descs[2], (nlay, h, vp, bad_vs, rho), noise, present[2])
    assert np.array_equal(got[2][rfonly], ref[2][rfonly]) and np.array_equal(bits(got[0][rfonly]), bits(ref[0][rfonly]))
    assert np.all(got[2][other] == 1)


# ---- chains ----------------------------------------------------------------------------------------------
CHAIN_KP = (21, 12, 30, 5)
CHAIN_KL = (15, 30, 8, 19)
CHAIN_KG = (9, 26, 14, 30)
CHAIN_P = (5.5, 6.4, 7.5, 6.0)
# slots and, per site, the slots it has.  PRIORS: the sigma of every dispersion slot and corr and sigma of the receiver function
# are free, so every site that lacks a slot lacks free noise parameters: its chains' set of free parameters is its own.
CHAIN_STRUCTURES = {
    "phase_rf": (("rph", "lph", "prf"), ["111", "110", "011", "101"]),
    "group": (("rph", "rgr", "prf"), ["111", "110", "101", "011"]),
}


def chain_slots(g, s, name):
    """site s of a chain structure: a list of targets with None where the site lacks the slot"""
    kinds, rows = CHAIN_STRUCTURES[name]
    rs = np.random.RandomState(500 + s)
    xs, ys = np.asarray(g["xsw"], dtype=float), np.asarray(g["ysw"], dtype=float)
    made = {}
    x1 = np.linspace(xs.min() + 0.3 * s, xs.max() - 1.1 * s, CHAIN_KP[s])
    made["rph"] = bh.RayleighDispersionPhase(x1, np.interp(x1, xs, ys) + rs.normal(0, 0.02, x1.size))
    x2 = np.linspace(xs.min() + 0.5 * s, xs.max() - 0.2 * s, CHAIN_KL[s])
    made["lph"] = bh.LoveDispersionPhase(x2, 1.05 * np.interp(x2, xs, ys) + rs.normal(0, 0.02, x2.size))
    x3 = np.linspace(xs.min() + 0.7 * s, xs.max() - 0.4 * s, CHAIN_KG[s])
    made["rgr"] = bh.RayleighDispersionGroup(x3, 0.9 * np.interp(x3, xs, ys) + rs.normal(0, 0.02, x3.size))
    t = bh.PReceiverFunction(g["xrf"], g["yrf"] + rs.normal(0, 0.01, g["yrf"].size))
    t.moddata.plugin.set_modelparams(gauss=1.0, p=CHAIN_P[s])
    made["prf"] = t
    return [made[k] if c == "1" else None for k, c in zip(kinds, rows[s])]


def own_targets(g, s, name):
    return bh.JointTarget([t for t in chain_slots(g, s, name) if t is not None])


def same_samples(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=True), "%s: %s" % (what, k)


@pytest.mark.parametrize("depth", [None, 1])
@pytest.mark.parametrize("name,search", [("phase_rf", "fast"), ("group", "reference")])
def test_chains_of_sites_that_lack_targets_walk_their_one_site_trajectories(name, search, depth, tmp_path):
    g = golden("chain_golden.npz")
    S, C = 4, 4
    init = dict(nchains=1, iter_burnin=150, iter_main=75, acceptance=(40, 80), thickmin=0.1, lvz=0.1, hvz=None, rcond=None,
                maxmodels=15, savepath=str(tmp_path / "multi"))
    names = ["st%d" % s for s in range(S)]
    st = bh.SiteTargets([chain_slots(g, s, name) for s in range(S)], names=names, per_site_x="all", per_site_rf=True, missing=True)
    dc = DeviceChains(st, C, init, PRIORS, seed=77, spec_depth=depth, search=search).run()
    assert dc.depth > 1 or depth == 1
    present = st.present
    # every site lacks free noise parameters or has them all; those that lack some still made noise moves (PAR_MAP: index 3)
    proposed = dc.state_host()["proposed"]
    assert (~present).any(axis=1).sum() == 3
    assert np.all(proposed[3] > 0), proposed[3]
    paths = dc.save() if depth is None else None
    for s in range(S):
        ip = dict(init, savepath=str(tmp_path / "one" / names[s]), station=names[s])
        one = DeviceChains(own_targets(g, s, name), C, ip, PRIORS, seed=77, chain_offset=s * C, spec_depth=depth, search=search).run()
        k = int(present[s].sum())
        for phase in ("p1", "p2"):
            a = dc.samples(phase, site=s)
            assert a["noise"].shape[-1] == 2 * k and a["misfits"].shape[-1] == k + 1
            same_samples(a, one.samples(phase), "%s site %d %s" % (name, s, phase))
        assert np.array_equal(dc.state_host()["proposed"][:, s * C:(s + 1) * C], one.state_host()["proposed"])
        if paths is not None:       # the saved folder of a site is that of its one-site run
            dpath = one.save()
            files = sorted(f for f in os.listdir(dpath) if f.endswith(".npy"))
            assert files and files == sorted(f for f in os.listdir(paths[s]) if f.endswith(".npy"))
            for f in files:
                assert np.array_equal(np.load(os.path.join(dpath, f)), np.load(os.path.join(paths[s], f)), equal_nan=True), f
            assert np.load(os.path.join(paths[s], "c%03d_p2noise.npy" % (s * C))).shape[-1] == 2 * k
            assert np.load(os.path.join(paths[s], "c%03d_p2misfits.npy" % (s * C))).shape[-1] == k + 1
            assert os.path.exists(os.path.join(paths[s], "%s_config.pkl" % names[s]))
            bh.save_final_distribution(paths[s], maxmodels=1000)
    # all chains at once: the slot layout, 0 where a site lacks the slot
    allc = dc.samples("p2")
    assert allc["noise"].shape[-1] == 2 * st.ntargets and allc["misfits"].shape[-1] == st.ntargets + 1
    for s in range(S):
        for t in np.flatnonzero(~present[s]):
            assert np.all(allc["misfits"][:, s * C:(s + 1) * C, t] == 0.0)


def test_tempered_chains_of_sites_that_lack_targets():
    g = golden("chain_golden.npz")
    S, C = 4, 4
    init = dict(nchains=1, iter_burnin=120, iter_main=60, acceptance=(40, 80), thickmin=0.1, lvz=0.1, hvz=None, rcond=None,
                maxmodels=10)
    betas = np.tile([1.0, 0.8, 1.0, 0.8], S)
    ladder = np.repeat(np.arange(2 * S), 2)                 # two ladders of two rungs per site
    st = bh.SiteTargets([chain_slots(g, s, "phase_rf") for s in range(S)], per_site_x="all", per_site_rf=True, missing=True)
    dc = DeviceChains(st, C, init, PRIORS, seed=9, betas=betas, ladder=ladder, swap_every=5).run()
    for s in range(S):
        blk = slice(s * C, (s + 1) * C)
        one = DeviceChains(own_targets(g, s, "phase_rf"), C, init, PRIORS, seed=9, chain_offset=s * C, betas=betas[blk],
                           ladder=ladder[blk], swap_every=5).run()
        same_samples(dc.samples("p2", site=s), one.samples("p2"), "tempered site %d" % s)
        same_samples(dc.samples("p2", site=s, cold_only=True), one.samples("p2", cold_only=True), "cold site %d" % s)
