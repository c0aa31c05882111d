"""The Rayleigh ellipticity with its own periods at every site, or absent at a site, on the MI355X
(include/bh_engine_sites_ellip.h, SiteTargets(per_site_ellip=True)).  The rule under test: a model of site s gets the logL, misfits,
err and synthetics of the EXISTING one-site fused call on the same engine -- JointTarget of the targets site s has, the ellipticity
fused -- whose ellipticity target has site s's periods; beyond a site's count and in the columns of a slot the site lacks the
synthetics are exact zeros, and an absent slot adds nothing, has misfit 0 and never sets err.  Bit for bit: no tolerance.  The
synthetics of a FAILED model are compared in their zeros only (include/bh_engine_ellip_target.h leaves its other columns open).
And a site of a DeviceChains walks the chain of its one-site DeviceChains."""
import ctypes as C

import numpy as np
import pytest

import bayhunter_amd as bh
from bayhunter_amd import engine as E
from bayhunter_amd.device_chains import DeviceChains
from bayhunter_amd.sites import slot_columns
from test_gpu_ellip_fused import MODELS70, B70, WATER, NOROOT, X7, XC, PRIORS, DINIT, bits, ellip, phase
from test_gpu_sites_missing import eval_device
from test_gpu_sites_x import configure
from test_gpu_swd_ellip import named

pytestmark = pytest.mark.gpu

NS = 4
SITE70 = (np.arange(B70) % NS).astype(np.int32)           # dealt round-robin: every wavefront mixes the sites
# "own": the ellipticity at 7, 3, 1 and 0 periods that are not the phase slot's; site 2 lacks the PHASE slot
OWN_ELL = (np.array([1.5, 2.5, 4.0, 7.0, 12.0, 21.0, 30.0]), np.array([2.2, 5.5, 13.0]), np.array([9.0]), None)
OWN_PH = (X7, X7[1:6], None, X7[:4])
# "shared": phase and ellipticity at the same periods per site, 7, 4 and 5 of them; site 3 is without the ellipticity
SH_X = (X7, np.array([2.5, 5.0, 9.0, 17.0]), np.array([1.2, 3.0, 6.5, 14.0, 27.0]), np.array([2.0, 4.0, 8.0]))
SH_ELL = SH_X[:3] + (None,)


def rows_of(ph, ell, **params):
    return [[None if ph[s] is None else phase(ph[s]), None if ell[s] is None else ellip(ell[s], True, **params)] for s in range(len(ph))]


def site_set(engine, ph, ell, **kw):
    return bh.SiteTargets(rows_of(ph, ell), engine=engine, per_site_x="all", missing=True, per_site_ellip=True, **kw)


CONFIGS = {"own": (OWN_PH, OWN_ELL), "shared": (SH_X, SH_ELL)}


def noise_slots(B):
    return np.tile(np.array([0.0, 0.05, 0.0, 0.07]), (B, 1))


def one_site(st, s, mods, noise):
    """the existing one-site fused call of site s on all the models: the targets it has, its own noise columns"""
    nlay, h, vp, vs, rho = mods
    return st.site(s).evaluate_batch(nlay, h, vp, vs, noise[:, slot_columns(st.present[s])[0]], rho=rho, want_ymod=True)


def layout(st):
    n = st._counts()
    return n, np.concatenate([[0], np.cumsum(n.max(axis=0))]).astype(int)


def assert_the_rule(got, ref, m, present_row, ns, off, what):
    """models m of one site against its one-site call: logL, err, the present misfits and the joint one bit for bit; the present
    columns of ymod bit for bit on the rows that did not fail; exact zeros beyond the site's count and in an absent slot's columns
    on every row; an absent slot's misfit 0.  Returns the number of unfailed models among m."""
    logL, misf, err, ymod = got
    _, mcol = slot_columns(present_row)
    assert np.array_equal(bits(logL[m]), bits(ref[0][m])), what + ": logL"
    assert np.array_equal(err[m], ref[2][m]), what + ": err"
    assert np.array_equal(bits(misf[m][:, mcol]), bits(ref[1][m])), what + ": misfits"
    ok = m & (ref[2] == 0)
    o = 0
    for t, has in enumerate(present_row):
        if not has:
            assert np.all(misf[m, t] == 0.0), "%s: misfit of absent slot %d" % (what, t)
            assert np.all(bits(ymod[m, off[t]:off[t + 1]]) == 0), "%s: columns of absent slot %d" % (what, t)
            continue
        k = ns[t]
        assert np.array_equal(bits(ymod[ok, off[t]:off[t] + k]), bits(ref[3][ok, o:o + k])), "%s: ymod of slot %d" % (what, t)
        assert np.all(bits(ymod[m, off[t] + k:off[t + 1]]) == 0), "%s: beyond the periods of slot %d" % (what, t)
        o += k
    assert o == ref[3].shape[1]
    return int(ok.sum())


def searches():
    yield "reference", ("reference", 0)
    yield "default", ("default", 32)


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_every_site_equals_its_one_site_fused_call(engine, config):
    """70 ragged models x a capacity of 7 = 490 lanes: two workgroups, model 36 across their boundary, every wavefront a mix of
    stations with 7, 3, 1 and 0 live lanes per model"""
    ph, ell = CONFIGS[config]
    mods = MODELS70
    nlay, h, vp, vs, rho = mods
    noise = noise_slots(B70)
    st = site_set(engine, ph, ell)
    n, off = layout(st)
    assert off[-1] == 14 and n[:, 1].tolist() == ([7, 3, 1, 0] if config == "own" else [7, 4, 5, 0])
    try:
        for name, setting in searches():
            configure(engine, *setting)
            refs = []
            for s in range(NS):
                refs.append(one_site(st, s, mods, noise))
                assert name == "reference" or engine.last_swd_kernel() == "lean"
            got = st.evaluate_batch(nlay, h, vp, vs, noise, SITE70, rho=rho, want_ymod=True)
            launches = engine.last_swd_launches()
            main = [l for l in launches if l["role"] == "main"]
            if name == "default":          # the trial-per-lane kernel: one launch; `interleaved` = two targets in it
                assert engine.last_swd_kernel() == "lean" and len(main) == 1
                assert main[0]["interleaved"] == (config == "own"), "%s: searches in the launch" % config
            dev = eval_device(engine, mods, noise, SITE70, engine.ldy)
            if config == "shared":         # no added search: the launches of the phase slot alone
                alone = bh.SiteTargets([[phase(x)] for x in SH_X], engine=engine, per_site_x="all", missing=True)
                alone.evaluate_batch(nlay, h, vp, vs, noise[:, :2], SITE70, rho=rho)
                assert engine.last_swd_launches() == launches
            unfailed = 0
            for s in range(NS):
                m = SITE70 == s
                unfailed += assert_the_rule(got, refs[s], m, st.present[s], n[s], off, "%s %s site %d host" % (config, name, s))
                assert_the_rule(dev, refs[s], m, st.present[s], n[s], off, "%s %s site %d device" % (config, name, s))
            failed = sorted(np.flatnonzero(got[2]))
            print("%s %s: %d of %d models unfailed at their site; failed: %r" % (config, name, unfailed, B70, failed))
            assert unfailed >= 60 and unfailed == B70 - len(failed)
    finally:
        engine.set_swd_trials(0)


def test_water_layer_and_rootless_models_where_the_count_is_short_and_where_it_is_zero(engine):
    """at site 1 (3 of 7 columns live) both fail as in the one-site call; at site 3, which lacks the ellipticity, the water-layer
    model is the phase slot's alone -- its search succeeds -- and the rootless one fails by the phase slot"""
    mods = MODELS70
    nlay, h, vp, vs, rho = mods
    noise = noise_slots(B70)
    st = site_set(engine, OWN_PH, OWN_ELL)
    n, off = layout(st)
    configure(engine, "reference", 0)
    refs = [one_site(st, s, mods, noise) for s in range(NS)]
    for where in (1, 3):
        site = SITE70.copy()
        site[[WATER, NOROOT]] = where
        got = st.evaluate_batch(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
        for s in range(NS):
            assert_the_rule(got, refs[s], site == s, st.present[s], n[s], off, "at site %d: site %d" % (where, s))
        logL, misf, err, ymod = got
        print("at site %d: err of the water-layer and the rootless model %d %d" % (where, err[WATER], err[NOROOT]))
        if where == 1:     # as in the one-site call: both fail
            assert err[WATER] == 1 and err[NOROOT] == 1 and logL[WATER] == -1e15
        else:              # the other slot's verdict alone (the search finds the water-layer model's roots)
            assert err[WATER] == refs[3][2][WATER] == 0 and err[NOROOT] == refs[3][2][NOROOT] and misf[WATER, 1] == 0.0
            assert np.all(bits(ymod[[WATER, NOROOT], off[1]:off[2]]) == 0)
        for b in (WATER, NOROOT):
            assert np.all(bits(ymod[b, off[1] + n[where, 1]:off[2]]) == 0)


def test_capacity_of_sixty_beside_one_period(engine):
    x60 = np.geomspace(1.0, 40.0, 60)
    ph, ell = (X7, X7), (x60, np.array([5.0]))
    models = [named("sediment"), named("crust"), named("lvz"), named("crust"), named("sediment")]
    mods = bh.pack_models(models)
    nlay, h, vp, vs, rho = mods
    site = np.array([0, 1, 1, 0, 1], dtype=np.int32)
    noise = noise_slots(5)
    st = bh.SiteTargets(rows_of(ph, ell), engine=engine, per_site_x="all", per_site_ellip=True)
    n, off = layout(st)
    assert n[:, 1].tolist() == [60, 1] and off[-1] == 67
    configure(engine, "reference", 0)
    refs = [one_site(st, s, mods, noise) for s in range(2)]
    got = st.evaluate_batch(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
    for s in range(2):
        assert assert_the_rule(got, refs[s], site == s, st.present[s], n[s], off, "capacity site %d" % s) >= 1
    ok = (site == 0) & (got[2] == 0)
    assert np.all(got[3][ok, 7:] != 0.0)


def test_a_site_out_of_range_on_the_device_entry_fails_in_band(engine):
    mods = MODELS70
    nlay, h, vp, vs, rho = mods
    noise = noise_slots(B70)
    st = site_set(engine, OWN_PH, OWN_ELL)
    configure(engine, "reference", 0)
    own = st.evaluate_batch(nlay, h, vp, vs, noise, SITE70, rho=rho, want_ymod=True)
    wild = SITE70.copy()
    wild[8], wild[44] = NS, -1
    dev = eval_device(engine, mods, noise, wild, engine.ldy)
    keep = np.ones(B70, bool)
    keep[[8, 44]] = False
    for k in (8, 44):
        assert dev[2][k] == 1 and dev[0][k] == -1e15 and np.all(dev[1][k] == 1e15) and np.all(bits(dev[3][k]) == 0)
    ok = keep & (own[2] == 0)
    for a, c in zip(dev[:3], own[:3]):
        assert np.array_equal(bits(a[keep]), bits(c[keep]))
    assert np.array_equal(bits(dev[3][ok]), bits(own[3][ok]))
    with pytest.raises(E.EngineError, match="out of range"):
        st.evaluate_batch(nlay, h, vp, vs, noise, wild, rho=rho)


def test_equal_periods_everywhere_give_the_existing_paths_bits(engine):
    """every site on one period set: through the table (the flag) what the shared-period path gives (no flag), with the phase slot
    at the ellipticity's periods (a shared search through the table, a private one on the existing path) and at others"""
    nlay, h, vp, vs, rho = MODELS70
    noise = noise_slots(B70)
    site = (np.arange(B70) % 3).astype(np.int32)
    for xph in (X7, OWN_ELL[0]):
        for name, setting in searches():
            configure(engine, *setting)
            out = []
            for flag in (True, False):
                st = bh.SiteTargets([[phase(xph), ellip(X7, True)] for _ in range(3)], engine=engine, per_site_x="all", per_site_ellip=flag)
                out.append(st.evaluate_batch(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True))
            engine.set_swd_trials(0)
            ok = out[1][2] == 0
            for k in range(3):
                assert np.array_equal(bits(out[0][k]), bits(out[1][k])), (name, k)
            assert np.array_equal(bits(out[0][3][ok]), bits(out[1][3][ok])) and ok.sum() >= 60


def test_argument_errors_and_refusals_change_nothing(engine):
    nlay, h, vp, vs, rho = MODELS70
    noise = noise_slots(B70)
    st = site_set(engine, OWN_PH, OWN_ELL)
    configure(engine, "reference", 0)
    before = st.evaluate_batch(nlay, h, vp, vs, noise, SITE70, rho=rho, want_ymod=True)
    L, hd = engine._L, engine._h
    last = lambda: L.bh_engine_last_error(hd).decode()
    for t, own, word in ((2, 1, "no such target"), (-1, 1, "no such target"), (0, 1, "not a BH_TARGET_ELLIP"), (1, 1, "a site table is in force"),
                         (1, 0, "a site table is in force")):
        assert L.bh_targets_set_ellip_sites(hd, t, own) == E.BH_EINVAL and word in last(), (t, own, last())
    cnt, x, yobs, yerr = st.site_x_arrays()
    P = lambda a: C.c_void_p(np.ascontiguousarray(a).ctypes.data)
    assert L.bh_sites_set(hd, NS, P(yobs), None) == E.BH_EINVAL and "bh_sites_set: an ellipticity target with periods per site" in last()
    assert L.bh_sites_set_x(hd, NS, P(cnt), P(x), P(yobs), None) == E.BH_EINVAL and "bh_sites_set_x: an ellipticity target with periods per site" in last()
    with pytest.raises(E.EngineError, match="bh_evaluate_sites"):
        engine.evaluate_batch(nlay, h, vp, vs, noise, rho=rho)
    after = engine.evaluate_sites(nlay, h, vp, vs, noise, SITE70, rho=rho, want_ymod=True)
    ok = before[2] == 0
    for k in range(3):
        assert np.array_equal(bits(before[k]), bits(after[k])), k
    assert np.array_equal(bits(before[3][ok]), bits(after[3][ok]))
    # the count table's rules for the flagged target: the dispersion target's
    descs = st._capacity_descs()

    def table(n_=cnt, x_=x, entry=L.bh_sites_set_missing):
        engine.set_targets(descs)
        return entry(hd, NS, P(np.ascontiguousarray(n_, dtype=np.int32)), P(x_), P(yobs), None)

    assert table(entry=L.bh_sites_set_x_all) == E.BH_EINVAL and "below 1" in last()      # a count of 0 from bh_sites_set_missing on
    b = cnt.copy()
    b[0, 1] = 8
    assert table(b) == E.BH_EINVAL and "capacity" in last()
    bx = x.copy()
    bx[1, 7 + 2] = -3.0
    assert table(x_=bx) == E.BH_EINVAL and "not finite and positive" in last()
    bx[1, 7 + 2], bx[1, 7 + 3] = x[1, 7 + 2], np.nan                                    # beyond the site's count: not read
    assert table(x_=bx) == E.BH_OK
    engine._owner = None
    again = st.evaluate_batch(nlay, h, vp, vs, noise, SITE70, rho=rho, want_ymod=True)
    for k in range(3):
        assert np.array_equal(bits(before[k]), bits(again[k])), k


# ---- chains -----------------------------------------------------------------------------------------------------------------------
CH_PH = (XC, np.array([3.0, 6.0, 10.0, 18.0]), np.array([2.0, 4.5, 8.0, 12.5, 25.0]))
CH_ELL = (np.array([2.5, 5.0, 9.0, 14.0, 22.0]), None, np.array([4.0, 8.0, 16.0]))


@pytest.fixture(scope="module")
def observed(engine):
    m = named("crust")
    with engine.searching("reference"), engine.computing("exact"):
        yd = bh.SurfDisp(XC, "rdispph", engine=engine).run_model(*m)[1]
        ye = bh.SurfEllip(XC, engine=engine).run_model(*m)[1]
    return yd, ye


def chain_row(observed, s, with_yerr=()):
    """site s of an array: the crust model's curves at the site's own periods, shifted a little per site; None: no ellipticity"""
    yd, ye = observed
    xd, xe = CH_PH[s], CH_ELL[s]
    td = bh.RayleighDispersionPhase(xd, np.interp(xd, XC, yd) * (1.0 + 0.004 * s))
    if xe is None:
        return [td, None]
    yerr = 0.01 + 0.002 * np.arange(xe.size) if s in with_yerr else None
    return [td, bh.RayleighEllipticity(xe, np.interp(xe, XC, ye) * (1.0 - 0.01 * s), yerr=yerr, fused=True)]


@pytest.mark.parametrize("laws", [False, True])
def test_site_chains_walk_the_one_site_runs(engine, observed, laws):
    """3 sites x 4 chains, 64 + 64 iterations; site 1 lacks the ellipticity.  laws: site 0's ellipticity has error bars
    (nocorr_scalederr), site 2's has none (nocorr)"""
    S, Cn = 3, 4
    yerr_at = (0,) if laws else ()
    sites = bh.SiteTargets([chain_row(observed, s, yerr_at) for s in range(S)], engine=engine, per_site_x="all", missing=True,
                           per_site_law=laws, per_site_ellip=True)
    dc = DeviceChains(sites, Cn, DINIT, PRIORS, seed=21).run()
    if laws:
        assert sites.site_law_arrays()[:, 1].tolist()[0::2] == [E.LAW_NOCORR_SCALED, E.LAW_NOCORR]
    for s in range(S):
        own = [t for t in chain_row(observed, s, yerr_at) if t is not None]
        one = DeviceChains(own, Cn, DINIT, PRIORS, seed=21, chain_offset=s * Cn).run()
        for ph in ("p1", "p2"):
            a, b = dc.samples(ph, site=s), one.samples(ph)
            assert set(a) == set(b)
            assert a["noise"].shape[-1] == 2 * len(own) and a["misfits"].shape[-1] == len(own) + 1
            for k in a:
                assert np.array_equal(a[k], b[k], equal_nan=True), "site %d %s: %s" % (s, ph, k)
        assert (one.state_host()["accepted"].sum(axis=0) > 0).all()
