"""Dispersion periods per site on every dispersion target (include/bh_engine_sites_x_all.h, SiteTargets(per_site_x="all")), the
parts that need no GPU: the header and the library's export, what SiteTargets accepts with "all" and still refuses with True,
the capacity descriptors and tables it registers, and -- with the oracle -- that the batches of the GPU tests are not about
zero rows."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, golden
import bayhunter_amd as bh
from bayhunter_amd.sites import SiteTargets
from test_sites_x_host import X_FULL, X_SETS, x_site, _RecordingEngine


def test_library_exports_the_site_x_all_header():
    from bayhunter_amd import engine as E
    txt = open(os.path.join(REPO, "include", "bh_engine_sites_x_all.h")).read()
    assert '#include "bh_engine_sites_x.h"' in txt
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decl = sorted(set(re.findall(r"\b(bh_[a-z_]+)\s*\(", txt)))
    assert decl == ["bh_sites_set_x_all"]
    assert sorted(E.SITE_X_ALL_SYMBOLS) == decl
    for other in (E.EXPORTED_SYMBOLS, E.DEBUG_SYMBOLS, E.SITE_SYMBOLS, E.SITE_RF_SYMBOLS, E.SITE_X_SYMBOLS, E.POSTERIOR_SYMBOLS):
        assert not set(decl) & set(other)
    lib = ctypes.CDLL(E.LIB_PATH)
    for name in decl:
        assert hasattr(lib, name), "missing export %s" % name
    for hdr in ("bh_engine.h", "bh_engine_debug.h", "bh_engine_sites.h", "bh_engine_sites_rf.h", "bh_engine_sites_x.h",
                "bh_engine_posterior.h"):                        # declared in the new header only
        assert "bh_sites_set_x_all" not in re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", hdr)).read(), flags=re.S)
    lib.bh_abi_version.restype = ctypes.c_int
    assert lib.bh_abi_version() == 10                            # extension headers are outside the contract


def test_all_accepts_differing_periods_on_group_and_higher_mode_targets_and_true_refuses_them():
    g = golden("chain_golden.npz")
    grp = [x_site(g, x, 0.01 * s, cls_r=bh.RayleighDispersionGroup) for s, x in enumerate(X_SETS)]
    md2 = [x_site(g, x, 0.01 * s, mode=2) for s, x in enumerate(X_SETS)]
    for sites in (grp, md2):
        st = SiteTargets(sites, per_site_x="all")
        st.check()
        assert st.per_site_x == "all"
        with pytest.raises(ValueError, match=r"x differs from site 0's on a group-velocity or higher-mode target \(per_site_x serves "
                                             r"fundamental-mode phase velocities\)"):
            SiteTargets(sites, per_site_x=True).check()
        with pytest.raises(ValueError, match=r"x differs from site 0's \(sites share x bit for bit\)"):
            SiteTargets(sites).check()
    assert SiteTargets(grp, per_site_x=True).per_site_x is True and SiteTargets(grp).per_site_x is False
    with pytest.raises(ValueError, match="per_site_x"):
        SiteTargets(grp, per_site_x="every")
    SiteTargets([x_site(g, x, p=5.5 + s, cls_r=bh.RayleighDispersionGroup) for s, x in enumerate(X_SETS)], per_site_x="all",
                per_site_rf=True).check()


def _rejects(sites, match, **kw):
    with pytest.raises(ValueError, match=match):
        SiteTargets(sites, per_site_x="all", **kw).check()


def test_all_keeps_the_other_refusals():
    g = golden("chain_golden.npz")
    G = bh.RayleighDispersionGroup
    a = x_site(g, X_FULL, cls_r=G)
    _rejects([a, x_site(g, X_SETS[1], cls_r=G, rfx=np.nextafter(np.asarray(g["xrf"], dtype=float), np.inf))], "x differs from site 0's")
    _rejects([a, x_site(g, np.linspace(2, 60, 61), cls_r=G)], "61 periods")
    _rejects([a, x_site(g, np.zeros(0), cls_r=G)], "0 periods")
    SiteTargets([a, x_site(g, np.geomspace(1, 40, 60), cls_r=G)], per_site_x="all").check()
    bad = X_SETS[1].copy()
    bad[3] = -bad[3]
    _rejects([a, x_site(g, bad, cls_r=G)], "not finite and positive")
    _rejects([x_site(g, x, law_sw="gauss", cls_r=G) for x in X_SETS[:2]], "Gauss law on a dispersion target")
    _rejects([a, x_site(g, X_SETS[1], law_sw="exp", cls_r=G)], "noise law")
    _rejects([a, x_site(g, X_SETS[1], p=7.0, cls_r=G)], "receiver-function parameters")
    _rejects([a, x_site(g, X_SETS[1], cls_r=G, mode=2)], "dispersion parameters")
    _rejects([a, x_site(g, X_SETS[1])], "is a RayleighDispersionPhase")


class _RecordingEngineAll(_RecordingEngine):
    def set_sites_x_all(self, n, x, yobs, yerr=None):
        self.calls.append(("sites_x_all", n.copy(), x.copy(), yobs.copy(), None if yerr is None else yerr.copy()))


def _two_curve_site(s, kp, kg, mode=None, yerr=False):
    """Rayleigh phase velocities at kp periods beside Love group velocities at kg periods"""
    x1, x2 = np.linspace(2.0 + s, 50.0, kp), np.linspace(3.0, 30.0 - s, kg)
    kw1 = {"yerr": 0.01 + 0.001 * np.arange(kp)} if yerr else {}
    kw2 = {"yerr": 0.02 + 0.001 * np.arange(kg)} if yerr else {}
    t1 = bh.RayleighDispersionPhase(x1, 3.4 + 0.01 * x1 + 0.01 * s, **kw1)
    t2 = bh.LoveDispersionGroup(x2, 3.2 + 0.02 * x2 + 0.01 * s, **kw2)
    if mode is not None:
        t2.moddata.plugin.set_modelparams(mode=mode)
    t1.set_noise_law("nocorr_scalederr" if yerr else "nocorr")
    t2.set_noise_law("nocorr_scalederr" if yerr else "exp")
    return bh.JointTarget([t1, t2])


@pytest.mark.parametrize("mode", [None, 3])
def test_registration_gives_every_dispersion_target_capacity_placeholders_and_calls_set_sites_x_all(mode):
    KP, KG = (7, 30, 1, 15), (12, 5, 26, 9)
    sites = [_two_curve_site(s, KP[s], KG[s], mode=mode, yerr=True) for s in range(4)]
    eng = _RecordingEngineAll()
    st = SiteTargets(sites, engine=eng, per_site_x="all")
    st._register()
    st._register()
    assert [c[0] for c in eng.calls] == ["targets", "sites_x_all"]
    descs = eng.calls[0][1]
    assert [d["n"] for d in descs] == [30, 26]
    for d in descs:                                 # placeholders on BOTH targets: the group target's x is never read either
        assert np.all(d["x"] == 1.0) and np.all(d["yobs"] == 0.0) and np.all(d["yerr"] == 1.0)
        assert np.size(d["x"]) == np.size(d["yobs"]) == np.size(d["yerr"]) == d["n"]
    assert descs[1]["igr"] == 1 and descs[1]["mode"] == (mode or 1) and descs[1]["iwave"] == 1
    _, n, x, yobs, yerr = eng.calls[1]
    assert n.dtype == np.int32 and np.array_equal(n, np.column_stack([KP, KG]))
    assert x.shape == yobs.shape == yerr.shape == (4, 56)
    for s, jt in enumerate(sites):
        for t, (off, cap) in enumerate(((0, 30), (30, 26))):
            k = n[s, t]
            assert np.array_equal(x[s, off:off + k], jt.targets[t].obsdata.x) and np.all(x[s, off + k:off + cap] == 0.0)
            assert np.array_equal(yobs[s, off:off + k], jt.targets[t].obsdata.y) and np.all(yobs[s, off + k:off + cap] == 0.0)
            assert np.array_equal(yerr[s, off:off + k], jt.targets[t].obsdata.yerr) and np.all(yerr[s, off + k:off + cap] == 1.0)
    # per_site_x=True on sites that share the group target's periods: its descriptor keeps them, and set_sites_x is called
    xs = np.linspace(3.0, 30.0, 12)
    shared = []
    for s in range(3):
        jt = _two_curve_site(s, KP[s], 12)
        jt.targets[1].obsdata.x = xs
        shared.append(jt)
    old = _RecordingEngineAll()
    SiteTargets(shared, engine=old, per_site_x=True)._register()
    assert [c[0] for c in old.calls] == ["targets", "sites_x"] and np.array_equal(old.calls[0][1][1]["x"], xs)
    new = _RecordingEngineAll()
    SiteTargets(shared, engine=new, per_site_x="all")._register()
    assert [c[0] for c in new.calls] == ["targets", "sites_x_all"] and np.all(new.calls[0][1][1]["x"] == 1.0)
    for a, b in zip(old.calls[1][1:4], new.calls[1][1:4]):      # the same tables either way
        assert np.array_equal(a, b)


def test_engine_method_passes_the_arrays_to_the_new_entry_point():
    """Engine.set_sites_x_all checks shapes as set_sites_x does and calls bh_sites_set_x_all (a stand-in library: no GPU)"""
    from bayhunter_amd import engine as E

    class Lib(object):
        def __init__(self):
            self.calls = []

        def bh_sites_set_x(self, *a):
            self.calls.append(("x", a[1]))
            return 0

        def bh_sites_set_x_all(self, *a):
            self.calls.append(("x_all", a[1]))
            return 0

    eng = E.Engine.__new__(E.Engine)
    eng._L, eng._h, eng.ldy, eng.ntargets = Lib(), None, 5, 2
    n = np.array([[2, 3], [1, 2], [2, 1]], np.int32)
    eng.set_sites_x_all(n, np.ones((3, 5)), np.zeros((3, 5)))
    eng.set_sites_x(n, np.ones((3, 5)), np.zeros((3, 5)))
    assert eng._L.calls == [("x_all", 3), ("x", 3)] and eng.nsites == 3
    with pytest.raises(ValueError, match="n must have shape"):
        eng.set_sites_x_all(n[:2], np.ones((3, 5)), np.zeros((3, 5)))
    with pytest.raises(ValueError, match="x must have the shape of yobs"):
        eng.set_sites_x_all(n, np.ones((3, 4)), np.zeros((3, 5)))


def test_the_gpu_tests_batches_are_not_about_zero_rows(oracle):
    """tests/test_gpu_sites_x_all.py compares whole rows, failed models and zero cells included.  For every (batch, site, target)
    it uses the oracle fails at most 30 % of the models and at least 50 % of the (model, period) cells are non-zero (a higher
    mode that does not exist at a period leaves a zero without a failure flag).  Fixed seeds: fixed shares."""
    from test_gpu_sites_x import batch, NSITES
    from test_gpu_sites_x_all import CASES, CASE_PARAMS, case_periods
    seen, worst_fail, least_cells = {}, 0.0, 1.0
    for case, family, Lmax in CASE_PARAMS:
        nlay, h, vp, vs, rho, site = batch(family, Lmax)
        assert min(np.bincount(site, minlength=NSITES)) >= 100
        for s in range(NSITES):
            m = site == s
            for t, (iwave, igr, mode, shift) in enumerate(CASES[case]["targets"]):
                per = case_periods(case, s, t)
                key = (family, Lmax, s, iwave, igr, mode, per.tobytes())
                if key not in seen:
                    v, e, _ = oracle.swd_batch(nlay[m], h.T[m], vp.T[m], vs.T[m], rho.T[m], per, iwave, igr, mode=mode)
                    seen[key] = float((e != 0).mean()), float((v != 0).mean())
                fail, cells = seen[key]
                worst_fail, least_cells = max(worst_fail, fail), min(least_cells, cells)
                assert fail <= 0.30, (case, family, Lmax, s, t, fail)
                assert cells >= 0.50, (case, family, Lmax, s, t, cells)
    from test_gpu_sites_x import PERIOD_SETS
    from test_gpu_sites_x_all import BIG_SHAPES, big_batch
    for B, _ in BIG_SHAPES:         # ... and the batches of one lane per second root
        nlay, h, vp, vs, rho, site = big_batch(B)
        for s, per in enumerate(PERIOD_SETS):
            m = site == s
            for iwave in (2, 1):
                v, e, _ = oracle.swd_batch(nlay[m], h.T[m], vp.T[m], vs.T[m], rho.T[m], per, iwave, 1)
                assert (e != 0).mean() <= 0.30 and (v != 0).mean() >= 0.50, (B, s, iwave, (e != 0).mean(), (v != 0).mean())
    assert worst_fail > 0.05 and least_cells < 1.0      # ... and failed models and zero cells do take part
