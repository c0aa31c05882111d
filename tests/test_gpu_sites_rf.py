"""Receiver-function parameters per site on the MI355X (include/bh_engine_sites_rf.h, SiteTargets(per_site_rf=True)):
bh_evaluate_sites with each site's own p and nsv against each site's own bh_evaluate_batch, bit for bit, on every coefficient
build; one trace against the extended-precision reference; the API's refusals; DeviceChains over such sites against one-site
runs."""
import pickle

import numpy as np
import pytest

from conftest import golden
import bayhunter_amd as bh
import rf_ref as RR
from bayhunter_amd import engine as E
from bayhunter_amd.device_chains import DeviceChains
from bayhunter_amd.synth import synth_models
from test_gpu_sites import eval_device, rinv_of

pytestmark = pytest.mark.gpu

# Six sites: p from 4 to 9 s/deg and one at 15 s/deg, where p = 0.135 s/km exceeds 1/vp of a half-space of 7.4 km/s and above
# (its P slowness is imaginary: the direct P wave's delay is NaN and the model fails in band; slower half-spaces stay real with
# post-critical interfaces above them -- the complex recursion next to the real one in one call).  nsv 0 (the model's top-layer
# vs) and > 0.
SITE_P = np.array([4.0, 5.5, 6.4, 7.5, 9.0, 15.0])
SITE_NSV = np.array([0.0, 2.0, 0.0, 1.5, 0.0, 3.0])
PER = np.linspace(3.0, 40.0, 12)


def rf_desc(law, waveno, n=201, nsamp=512, fsamp=5.0):
    d = dict(kind=E.TARGET_RF, law=law, n=n, waveno=waveno, nsamp=nsamp, p=6.4, gauss=2.5, fsamp=fsamp, tshift=5.0, nsv=0.0)
    if law == E.LAW_GAUSS:
        d["rinv"], d["logdet_r"] = rinv_of(n)
    return d


def structure(case):
    """target descriptors without observed data"""
    if case == "exp_P":             # P, exponential law
        return [rf_desc(E.LAW_EXP, 0)]
    if case == "nocorr_SV":         # SV, nocorr law; a P trace beside it
        return [rf_desc(E.LAW_NOCORR, 1), rf_desc(E.LAW_EXP, 0, n=150)]
    if case == "gauss":             # the Gauss law on P and SV
        return [rf_desc(E.LAW_GAUSS, 0, n=100), rf_desc(E.LAW_GAUSS, 1, n=100)]
    if case == "long":              # nsamp 32768 > 16384: the spectrum in the HBM workspace
        return [rf_desc(E.LAW_EXP, 1, n=400, nsamp=32768, fsamp=20.0)]
    if case == "joint":             # beside a dispersion target: the start gate, the coefficient kernel's _small build
        return [dict(kind=E.TARGET_SWD, law=E.LAW_NOCORR, n=12, x=PER, iwave=2, igr=0),
                rf_desc(E.LAW_EXP, 0), rf_desc(E.LAW_NOCORR, 1, n=120)]
    raise KeyError(case)


def site_descs(case, rs):
    """every site: the structure with its own observed data and, per receiver function, its own p and nsv (the receiver
    functions of one site differ by 0.25 s/deg, so that a wrong table column shows)"""
    out = []
    for s in range(len(SITE_P)):
        ds, k = [], 0
        for d in structure(case):
            d = dict(d)
            n = d["n"]
            if d["kind"] == E.TARGET_SWD:
                d["yobs"] = 3.0 + 0.02 * np.arange(n) + rs.normal(0, 0.05, n)
            else:
                d["yobs"] = rs.normal(0, 0.05, n)
                d["p"], d["nsv"] = float(SITE_P[s] + 0.25 * k), float(SITE_NSV[s])
                k += 1
            ds.append(d)
        out.append(ds)
    return out


def tables(descs):
    """(yobs[S, ldy], p[S, nt], nsv[S, nt]) of site descriptors (p, nsv: 0 in the columns of other targets)"""
    yobs = np.vstack([np.concatenate([d["yobs"] for d in ds]) for ds in descs])
    p = np.array([[d["p"] if d["kind"] == E.TARGET_RF else 0.0 for d in ds] for ds in descs])
    nsv = np.array([[d["nsv"] if d["kind"] == E.TARGET_RF else 0.0 for d in ds] for ds in descs])
    return yobs, p, nsv


def models(rs, B, Lmax):
    nlay, h, vp, vs, rho = synth_models(rs, B, Lmax, ragged=True)
    nlay[0] = Lmax
    return nlay, h, vp, vs, rho


def per_site(eng, descs, mods, noise):
    out = []
    for ds in descs:
        eng.set_targets(ds)
        out.append(eng.evaluate_batch(*mods[:4], noise, rho=mods[4], want_ymod=True))
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same_bits(got, ref, what):
    """(logL, misfits, err, ymod) of the same models, bit for bit: a NaN trace gives a NaN logL on both paths"""
    for k, (x, y) in enumerate(zip(got, ref)):
        if k == 3:
            ok = got[2] == 0
            x, y = x[ok], y[ok]
        assert np.array_equal(bits(x), bits(y)), "%s: %s" % (what, ("logL", "misfits", "err", "ymod")[k])


def assert_sites_equal(got, refs, site, what):
    for s, ref in enumerate(refs):
        m = site == s
        same_bits([a[m] for a in got], [a[m] for a in ref], "%s, site %d" % (what, s))


def failed(got):
    """models failed in band (err) or with a NaN trace (NaN logL, as the reference's likelihood of a NaN trace)"""
    return (got[2] != 0) | ~np.isfinite(got[0])


def register(eng, descs):
    yobs, p, nsv = tables(descs)
    eng.set_targets(descs[0])
    eng.set_sites(yobs)
    eng.set_sites_rf(p, nsv)


# Lmax 8 / 21 / 40: rf_coef_layers_sites_kernel<16> / <32> / rf_coef_sites_kernel; "joint" at 12 / 24 runs
# rf_coef_layers_sites_kernel_small<16> / <32> behind the start gate (the engine does not report the build; a kernel trace of
# this test shows it).
@pytest.mark.parametrize("case,Lmax", [("exp_P", 8), ("nocorr_SV", 21), ("gauss", 40), ("exp_P", 40), ("long", 8),
                                       ("joint", 12), ("joint", 24)])
def test_per_site_rf_equals_each_sites_own_evaluation(engine, case, Lmax):
    rs = np.random.RandomState(Lmax + 7 * len(case))
    descs = site_descs(case, rs)
    nt, S, B = len(descs[0]), len(descs), 150
    mods = models(rs, B, Lmax)
    noise = np.column_stack([rs.uniform(0.1, 0.6, B) if i % 2 == 0 else rs.uniform(0.02, 0.1, B) for i in range(2 * nt)])
    site = rs.randint(0, S, B).astype(np.int32)
    refs = per_site(engine, descs, mods, noise)
    register(engine, descs)
    got = engine.evaluate_sites(*mods[:4], noise, site, rho=mods[4], want_ymod=True)
    assert_sites_equal(got, refs, site, "%s Lmax %d host" % (case, Lmax))
    assert_sites_equal(eval_device(engine, mods, noise, site, engine.ldy), refs, site, "%s Lmax %d device" % (case, Lmax))
    bad = failed(got)
    if case in ("exp_P", "joint"):      # the P wave at 15 s/deg: some models fail (NaN trace), others not
        m = site == 5
        assert bad[m].any() and not bad[m].all()
    # the sites differ: a model of site 0 has another trace with site 4's p
    assert not np.array_equal(refs[0][3][~bad], refs[4][3][~bad])


def test_site_trace_against_the_reference(engine):
    """traces of the site with p = 9 s/deg, nsv = 1.5 km/s against tests/rf_ref.py: 1e-9 of the peak"""
    rs = np.random.RandomState(21)
    descs = site_descs("nocorr_SV", rs)
    nt, B = len(descs[0]), 24
    mods = models(rs, B, 10)
    noise = np.tile([0.0, 0.05, 0.4, 0.05], (B, 1))
    site = np.full(B, 4, np.int32)
    site[::3] = 1
    register(engine, descs)
    _, _, err, ymod = engine.evaluate_sites(*mods[:4], noise, site, rho=mods[4], want_ymod=True)
    off = 0
    for d in descs[4]:
        m = site == 4
        nl, h, vp, vs, rho = mods[0][m], mods[1][:, m], mods[2][:, m], mods[3][:, m], mods[4][:, m]
        ref = RR.rf_ref(nl, h, vp, vs, rho, d["p"], d["gauss"], d["nsamp"], d["fsamp"], d["tshift"], d["waveno"], d["n"],
                        nsv=d["nsv"])
        want = np.asarray(ref.rf, dtype=np.float64)
        got = ymod[m, off:off + d["n"]]
        ok = np.all(np.isfinite(want), axis=1)
        assert ok.sum() >= 8
        assert np.array_equal(np.all(np.isfinite(got), axis=1), ok)
        peak = np.max(np.abs(want[ok]))
        assert np.max(np.abs(got[ok] - want[ok])) <= 1e-9 * peak, (d["waveno"], np.max(np.abs(got[ok] - want[ok])) / peak)
        off += d["n"]


def test_api_refusals_and_lifetime(engine):
    rs = np.random.RandomState(4)
    descs = site_descs("nocorr_SV", rs)
    nt, B = len(descs[0]), 60
    mods = models(rs, B, 10)
    noise = np.tile([0.0, 0.05, 0.4, 0.05], (B, 1))
    site = rs.randint(0, len(descs), B).astype(np.int32)
    yobs, p, nsv = tables(descs)
    L, h = engine._L, engine._h
    P = lambda a: a.ctypes.data
    engine.set_targets(descs[0])
    assert L.bh_sites_set_rf(h, len(descs), P(p), P(nsv)) == E.BH_EINVAL          # no site table yet
    engine.set_sites(yobs)
    shared = engine.evaluate_sites(*mods[:4], noise, site, rho=mods[4], want_ymod=True)
    assert L.bh_sites_set_rf(h, len(descs) - 1, P(p), P(nsv)) == E.BH_EINVAL      # another number of sites
    assert L.bh_sites_set_rf(h, len(descs), None, P(nsv)) == E.BH_EINVAL
    assert L.bh_sites_set_rf(h, len(descs), P(p), None) == E.BH_EINVAL
    for bad in (np.nan, np.inf):
        for a in (p, nsv):
            b = a.copy()
            b[2, 1] = bad
            with pytest.raises(E.EngineError, match="non-finite"):
                engine.set_sites_rf(b if a is p else p, b if a is nsv else nsv)
    batch0 = engine.evaluate_batch(*mods[:4], noise, rho=mods[4], want_ymod=True)
    engine.set_sites_rf(p, nsv)
    own = engine.evaluate_sites(*mods[:4], noise, site, rho=mods[4], want_ymod=True)
    assert not np.array_equal(own[3], shared[3])
    same_bits(engine.evaluate_batch(*mods[:4], noise, rho=mods[4], want_ymod=True), batch0, "evaluate_batch")  # not read
    engine.set_sites(yobs)                     # set_sites drops the table: the descriptor's p and nsv again
    same_bits(engine.evaluate_sites(*mods[:4], noise, site, rho=mods[4], want_ymod=True), shared, "after set_sites")
    engine.set_sites_rf(p, nsv)
    engine.set_targets(descs[0])               # set_targets drops both tables
    with pytest.raises(E.EngineError, match="site table"):
        engine.set_sites_rf(p, nsv)


# ---- chains ----------------------------------------------------------------------------------------------
PRIORS = dict(vpvs=(1.4, 2.1), layers=(1, 10), vs=(2, 5), z=(0, 60), rfnoise_corr=(0.35, 0.75),
              rfnoise_sigma=(1e-5, 0.05), swdnoise_corr=0., swdnoise_sigma=(1e-5, 0.1))
CHAIN_P = (5.5, 6.4, 7.5)
CHAIN_NSV = (None, 2.0, None)


def chain_site(g, s):
    rs = np.random.RandomState(300 + s)
    t1 = bh.RayleighDispersionPhase(g["xsw"], g["ysw"] + rs.normal(0, 0.02, g["ysw"].size))
    t2 = bh.PReceiverFunction(g["xrf"], g["yrf"] + rs.normal(0, 0.01, g["yrf"].size))
    t2.moddata.plugin.set_modelparams(gauss=1.0, p=CHAIN_P[s], nsv=CHAIN_NSV[s])
    return bh.JointTarget([t1, t2])


class _RefUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if module.startswith("BayHunter"):
            return type(name, (object,), {})
        return super().find_class(module, name)


@pytest.mark.parametrize("depth", [None, 1])
def test_per_site_rf_chains_walk_the_one_site_trajectories(depth, tmp_path):
    g = golden("chain_golden.npz")
    S, C = 3, 4
    init = dict(nchains=1, iter_burnin=150, iter_main=75, acceptance=(40, 80), thickmin=0.1, lvz=0.1, hvz=None, rcond=None,
                maxmodels=15, savepath=str(tmp_path / "multi"))
    st = bh.SiteTargets([chain_site(g, s) for s in range(S)], names=["st%d" % s for s in range(S)], per_site_rf=True)
    dc = DeviceChains(st, C, init, PRIORS, seed=77, spec_depth=depth).run()
    for s in range(S):
        one = DeviceChains(chain_site(g, s), C, init, PRIORS, seed=77, chain_offset=s * C, spec_depth=depth).run()
        for phase in ("p1", "p2"):
            a, b = dc.samples(phase, site=s), one.samples(phase)
            for k in a:
                assert np.array_equal(a[k], b[k], equal_nan=True), "site %d %s: %s" % (s, phase, k)
    if depth is None:
        paths = dc.save()
        for s in range(S):
            with open("%s/st%d_config.pkl" % (paths[s], s), "rb") as f:
                cfg = _RefUnpickler(f).load()
            mp = cfg["targets"][1].moddata.plugin.modelparams
            assert mp["p"] == CHAIN_P[s] and mp["nsv"] == CHAIN_NSV[s]
