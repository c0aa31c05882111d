"""Dispersion periods per site (include/bh_engine_sites_x.h, SiteTargets(per_site_x=True)), the parts that need no GPU: the
header and the library's export, what SiteTargets accepts and rejects, the padded tables it builds, what it registers, the
LDS the group kernel's plan asks for with periods per model, and the failure shares of the GPU tests' batches."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, golden
import bayhunter_amd as bh
from bayhunter_amd.sites import SiteTargets

X_FULL = np.linspace(2, 60, 30)
X_SETS = [X_FULL, X_FULL[::2].copy(), np.array([1.0, 1.7, 2.9, 4.0, 6.5, 8.1, 11.0]), np.array([7.5])]


def x_site(g, x, dy=0.0, rf=True, law_sw="nocorr", love=True, yerr=False, p=6.4, rfx=None, cls_r=None, mode=None, corr=0.5):
    x = np.asarray(x, dtype=float)
    kw = {"yerr": 0.01 + 0.001 * np.arange(x.size)} if yerr else {}
    ts = [(cls_r or bh.RayleighDispersionPhase)(x, 3.4 + 0.01 * x + dy, **kw)]
    if love:
        ts.append(bh.LoveDispersionPhase(x, 3.7 + 0.012 * x + dy, **kw))
    if mode is not None:
        ts[0].moddata.plugin.set_modelparams(mode=mode)
    for t in ts:
        t.set_noise_law(law_sw, corr=corr, rcond=1e-5) if law_sw == "gauss" else t.set_noise_law(law_sw)
    if rf:
        t = bh.PReceiverFunction(g["xrf"] if rfx is None else rfx, g["yrf"] * (1.0 + dy))
        t.moddata.plugin.set_modelparams(gauss=1.0, p=p)
        t.set_noise_law("exp")
        ts.append(t)
    return bh.JointTarget(ts)


def test_library_exports_the_site_x_header():
    from bayhunter_amd import engine as E
    txt = open(os.path.join(REPO, "include", "bh_engine_sites_x.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decl = sorted(set(re.findall(r"\b(bh_[a-z_]+)\s*\(", txt)))
    assert decl == ["bh_sites_set_x"]
    assert sorted(E.SITE_X_SYMBOLS) == decl
    for other in (E.EXPORTED_SYMBOLS, E.DEBUG_SYMBOLS, E.SITE_SYMBOLS, E.SITE_RF_SYMBOLS, E.POSTERIOR_SYMBOLS):
        assert not set(decl) & set(other)
    lib = ctypes.CDLL(E.LIB_PATH)
    for name in decl:
        assert hasattr(lib, name), "missing export %s" % name
    for hdr in ("bh_engine.h", "bh_engine_debug.h", "bh_engine_sites.h", "bh_engine_sites_rf.h"):   # declared in the new header only
        assert "bh_sites_set_x" not in re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", hdr)).read(), flags=re.S)


def test_per_site_x_accepts_differing_periods_and_the_default_refuses_them():
    g = golden("chain_golden.npz")
    sites = [x_site(g, x, 0.01 * s) for s, x in enumerate(X_SETS)]
    st = SiteTargets(sites, per_site_x=True)
    st.check()
    assert st.per_site_x and not SiteTargets(sites).per_site_x
    with pytest.raises(ValueError, match=r"x differs from site 0's \(sites share x bit for bit\)"):
        SiteTargets(sites).check()
    with pytest.raises(ValueError, match=r"site 1 \(site001\), target 0 \(rdispph\): x differs from site 0's \(sites share x bit for bit\)"):
        SiteTargets(sites[:2], per_site_rf=True).check()
    SiteTargets([x_site(g, X_FULL, 0.01 * s) for s in range(3)], per_site_x=True).check()      # shared x stays fine
    SiteTargets([x_site(g, x, p=5.5 + s) for s, x in enumerate(X_SETS)], per_site_x=True, per_site_rf=True).check()


def _rejects(sites, match, **kw):
    with pytest.raises(ValueError, match=match):
        SiteTargets(sites, per_site_x=True, **kw).check()


def test_per_site_x_rejects_what_the_engine_refuses():
    g = golden("chain_golden.npz")
    a = x_site(g, X_FULL)
    # a receiver function's x stays shared bit for bit
    _rejects([a, x_site(g, X_SETS[1], rfx=np.nextafter(np.asarray(g["xrf"], dtype=float), np.inf))], "x differs from site 0's")
    # group velocities and higher modes: only with site 0's x
    grp = [x_site(g, x, cls_r=bh.RayleighDispersionGroup) for x in X_SETS[:2]]
    _rejects(grp, "group-velocity or higher-mode")
    _rejects([x_site(g, x, mode=2) for x in X_SETS[:2]], "group-velocity or higher-mode")
    SiteTargets([x_site(g, X_FULL, 0.01 * s, cls_r=bh.RayleighDispersionGroup) for s in range(2)], per_site_x=True).check()
    SiteTargets([x_site(g, X_FULL, 0.01 * s, mode=2) for s in range(2)], per_site_x=True).check()
    # 1 to 60 periods
    _rejects([a, x_site(g, np.linspace(2, 60, 61))], "61 periods")
    _rejects([x_site(g, np.linspace(2, 60, 61)), a], "61 periods")
    _rejects([a, x_site(g, np.zeros(0))], "0 periods")
    SiteTargets([a, x_site(g, np.geomspace(1, 40, 60))], per_site_x=True).check()
    # periods are finite and positive
    bad = X_SETS[1].copy()
    bad[3] = -bad[3]
    _rejects([a, x_site(g, bad)], "not finite and positive")
    bad[3] = np.inf
    _rejects([a, x_site(g, bad)], "not finite and positive")
    # the Gauss law's R^-1 depends on the number of samples
    _rejects([x_site(g, x, law_sw="gauss") for x in X_SETS[:2]], "Gauss law on a dispersion target")
    # the other mismatches are refused as before
    _rejects([a, x_site(g, X_SETS[1], law_sw="exp")], "noise law")
    _rejects([a, x_site(g, X_SETS[1], p=7.0)], "receiver-function parameters")
    _rejects([a, x_site(g, X_SETS[1], rf=False)], "targets")


def test_site_x_arrays_layout_padding_and_counts():
    g = golden("chain_golden.npz")
    nrf = np.size(g["xrf"])
    sites = [x_site(g, x, 0.01 * s, law_sw="nocorr_scalederr", yerr=True) for s, x in enumerate(X_SETS)]
    n, x, yobs, yerr = SiteTargets(sites, per_site_x=True).site_x_arrays()
    assert n.dtype == np.int32 and np.array_equal(n, [[30, 30, nrf], [15, 15, nrf], [7, 7, nrf], [1, 1, nrf]])
    ldy = 30 + 30 + nrf
    assert x.shape == yobs.shape == yerr.shape == (4, ldy)
    for s, (jt, xs) in enumerate(zip(sites, X_SETS)):
        k = xs.size
        for t, off in enumerate((0, 30)):
            assert np.array_equal(x[s, off:off + k], xs) and np.all(x[s, off + k:off + 30] == 0.0)
            assert np.array_equal(yobs[s, off:off + k], jt.targets[t].obsdata.y) and np.all(yobs[s, off + k:off + 30] == 0.0)
            assert np.array_equal(yerr[s, off:off + k], jt.targets[t].obsdata.yerr) and np.all(yerr[s, off + k:off + 30] == 1.0)
        assert np.array_equal(x[s, 60:], g["xrf"]) and np.array_equal(yobs[s, 60:], jt.targets[2].obsdata.y)
    # no scaled-error law: no yerr table; the capacity is the largest count, whichever site has it
    n, x, yobs, yerr = SiteTargets([x_site(g, X_SETS[2], rf=False), x_site(g, X_SETS[1], rf=False)], per_site_x=True).site_x_arrays()
    assert yerr is None and x.shape == (2, 30) and np.array_equal(n, [[7, 7], [15, 15]])
    assert np.array_equal(x[0, 15:22], X_SETS[2]) and np.array_equal(x[1, 15:], X_SETS[1])


class _RecordingEngine(object):
    """what SiteTargets._register asks of an engine, recorded"""

    def __init__(self):
        self._owner = None
        self.calls = []

    def set_targets(self, descs):
        self.calls.append(("targets", [dict(d) for d in descs]))

    def set_sites(self, yobs, yerr=None):
        self.calls.append(("sites", yobs.copy()))

    def set_sites_x(self, n, x, yobs, yerr=None):
        self.calls.append(("sites_x", n.copy(), x.copy(), yobs.copy(), None if yerr is None else yerr.copy()))

    def set_sites_rf(self, p, nsv):
        self.calls.append(("sites_rf", np.array(p, dtype=float), np.array(nsv, dtype=float)))


def test_registration_passes_capacity_descriptors_and_the_tables():
    g = golden("chain_golden.npz")
    eng = _RecordingEngine()
    order = [2, 0, 3, 1]                                       # site 0 is not the one with the most periods
    st = SiteTargets([x_site(g, X_SETS[k], 0.01 * s, p=5.5 + s) for s, k in enumerate(order)], engine=eng, per_site_x=True,
                     per_site_rf=True)
    st._register()
    st._register()
    assert [c[0] for c in eng.calls] == ["targets", "sites_x", "sites_rf"]
    descs = eng.calls[0][1]
    assert [d["n"] for d in descs[:2]] == [30, 30] and all(np.size(d["x"]) == 30 and np.size(d["yobs"]) == 30 for d in descs[:2])
    assert descs[2]["n"] == np.size(g["xrf"]) and descs[2]["p"] == 5.5
    _, n, x, yobs, yerr = eng.calls[1]
    assert np.array_equal(n[:, 0], [7, 30, 1, 15]) and yerr is None and np.array_equal(x[1, :30], X_FULL)
    # replacing one site's x array registers again (the signature holds the arrays by identity)
    sig = st._signature()
    st.site(3).targets[0].obsdata.x = X_SETS[1][:12].copy()
    st.site(3).targets[0].obsdata.y = st.site(3).targets[0].obsdata.y[:12].copy()
    assert st._signature() != sig
    st._register()
    assert [c[0] for c in eng.calls[3:]] == ["targets", "sites_x", "sites_rf"] and eng.calls[4][1][3, 0] == 12
    plain = _RecordingEngine()                                 # the default: site 0's descriptors and the plain table
    SiteTargets([x_site(g, X_FULL, 0.01 * s) for s in range(2)], engine=plain)._register()
    assert [c[0] for c in plain.calls] == ["targets", "sites"] and np.array_equal(plain.calls[0][1][0]["x"], X_FULL)


def test_group_plan_sizes_lds_for_periods_per_model():
    """bh_plan_swd_group with SwdGroupAsk::sitex (reached as tests/test_swd_group_plan.py reaches the plan): a wavefront's region
    holds a row of K periods for each of its models instead of one, the same build is named, and one model per wavefront
    (a sampler's window, the re-run) asks for nothing more.  Without the flag the plan is what it was."""
    import ctypes as C
    import test_swd_group_plan as P

    class Ask(C.Structure):  # SwdGroupAsk with its sitex flag (bh_device.h)
        _fields_ = [("B", C.c_int), ("Lmax", C.c_int), ("Lcut", C.c_int), ("ntargets", C.c_int), ("G0", C.c_int), ("t", P.Target * 8),
                    ("fast", C.c_bool), ("farith", C.c_bool), ("restart", C.c_bool), ("adapt_ok", C.c_bool), ("rerun", C.c_bool),
                    ("counters", C.c_bool), ("sitex", C.c_bool), ("scan", C.c_int)]

    assert C.sizeof(Ask) == C.sizeof(P.Ask) and Ask.scan.offset == P.Ask.scan.offset
    plan, tun, _, _ = P.library()

    def ask(B, Lmax, K, sitex, G0=4, look=1, adapt_ok=False):
        q = Ask(B=B, Lmax=Lmax, Lcut=Lmax, ntargets=1, G0=G0, restart=True, adapt_ok=adapt_ok, sitex=sitex)
        q.t[0] = P.Target(K=K, look=look, iwave=P.R, mode=1)
        return plan(C.cast(C.byref(q), C.POINTER(P.Ask)), tun)

    def key(g):
        b = g.build
        return (b.fastm, b.simple, b.prof, b.adapt, b.cntb, b.fa)

    for K in (1, 7, 30, 60):
        a, b = ask(4096, 10, K, False), ask(4096, 10, K, True)
        assert a.fits and b.fits and key(a) == key(b)
        if a.lanes[1] == b.lanes[1]:
            mpw = 64 // a.lanes[1]
            assert b.wave_lds - a.wave_lds == 8 * ((K + 1) & ~1) * (mpw - 1), (K, a.wave_lds, b.wave_lds)
        else:       # the rows did not fit the residency target: fewer models per wavefront
            assert b.lanes[1] > a.lanes[1]
        a, b = ask(64, 10, K, False, G0=16, look=4, adapt_ok=True), ask(64, 10, K, True, G0=16, look=4, adapt_ok=True)
        assert a.build.adapt and b.build.adapt and a.wave_lds == b.wave_lds and a.lds == b.lds and key(a) == key(b)
    assert ask(4096, 10, 60, True).wave_lds > ask(4096, 10, 60, False).wave_lds


def test_the_gpu_tests_batches_fail_on_fewer_than_30_percent_of_any_site(oracle):
    """tests/test_gpu_sites_x.py compares whole rows, failed models included; so that it is not about zero rows, at most 30 % of
    the models of any (batch, site, wave type) fail in the oracle (fixed seeds: fixed shares, checked here without a GPU)."""
    from test_gpu_sites_x import batch, PERIOD_SETS, FAMILIES, LMAX
    worst = 0.0
    for family in FAMILIES:
        for Lmax in LMAX:
            nlay, h, vp, vs, rho, site = batch(family, Lmax)
            assert min(np.bincount(site, minlength=len(PERIOD_SETS))) >= 100
            for s, per in enumerate(PERIOD_SETS):
                m = site == s
                for iwave in (2, 1):
                    _, e, _ = oracle.swd_batch(nlay[m], h.T[m], vp.T[m], vs.T[m], rho.T[m], per, iwave, 0)
                    share = float((e != 0).mean())
                    worst = max(worst, share)
                    assert share <= 0.30, (family, Lmax, s, iwave, share)
    assert worst > 0.05         # ... and failed models do take part


def test_shared_group_velocity_and_higher_mode_targets_keep_their_periods_in_the_descriptor():
    """A target that per-site periods are not built for keeps site 0's x in its capacity descriptor: the engine checks the
    table against it and searches a group velocity's second roots there.  The phase-velocity target beside it gets placeholders."""
    g = golden("chain_golden.npz")
    xs = np.linspace(3.0, 30.0, 12)
    for kw in (dict(cls=bh.LoveDispersionGroup), dict(cls=bh.LoveDispersionPhase, mode=2)):
        sites = []
        for s, x in enumerate(X_SETS[:3]):
            t1 = bh.RayleighDispersionPhase(x, 3.4 + 0.01 * x)
            t2 = kw["cls"](xs, 3.7 + 0.01 * xs + 0.01 * s)
            if "mode" in kw:
                t2.moddata.plugin.set_modelparams(mode=kw["mode"])
            t1.set_noise_law("nocorr")
            t2.set_noise_law("exp")
            sites.append(bh.JointTarget([t1, t2]))
        eng = _RecordingEngine()
        st = SiteTargets(sites[::-1], engine=eng, per_site_x=True)
        st._register()
        descs, (_, n, x, yobs, yerr) = eng.calls[0][1], eng.calls[1]
        assert descs[0]["n"] == 30 and np.all(descs[0]["x"] == 1.0)
        assert descs[1]["n"] == 12 and np.array_equal(descs[1]["x"], xs) and np.array_equal(descs[1]["yobs"], sites[2].targets[1].obsdata.y)
        assert np.array_equal(n, [[7, 12], [15, 12], [30, 12]]) and all(np.array_equal(x[s, 30:], xs) for s in range(3))
