"""Many stations at once (bayhunter_amd/sites.py, include/bh_engine_sites.h), the parts that need no GPU: what SiteTargets
accepts and rejects, the column -> site map of a speculative window, and the exported symbols of the site header."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, golden
import bayhunter_amd as bh
from bayhunter_amd.sites import SiteTargets, window_site_map


def site_targets(g, dy=0.0, law_rf="exp", law_sw="nocorr", yerr=None, mode=None, p=6.4, corr=0.9):
    t1 = bh.RayleighDispersionPhase(g["xsw"], g["ysw"] + dy, yerr=yerr)
    t2 = bh.PReceiverFunction(g["xrf"], g["yrf"] * (1.0 + dy))
    t2.moddata.plugin.set_modelparams(gauss=1.0, p=p)
    if mode is not None:
        t1.moddata.plugin.set_modelparams(mode=mode)
    t1.set_noise_law(law_sw)
    t2.set_noise_law(law_rf, corr=corr, rcond=1e-5) if law_rf == "gauss" else t2.set_noise_law(law_rf)
    return bh.JointTarget([t1, t2])


def test_sites_that_differ_in_y_and_yerr_are_accepted():
    g = golden("chain_golden.npz")
    err = np.abs(g["ysw_err"]) + 0.01
    sites = [site_targets(g, dy=0.01 * s, law_sw="nocorr_scalederr", yerr=err * (1 + 0.1 * s)) for s in range(3)]
    st = SiteTargets(sites, names=["A", "B", "C"])
    st.check()
    yobs, yerr = st.site_arrays()
    assert yobs.shape == yerr.shape == (3, 21 + 201)
    assert np.array_equal(yobs[2, :21], g["ysw"] + 0.02) and np.array_equal(yerr[1, :21], err * 1.1)
    assert st.nsites == 3 and st.names == ["A", "B", "C"] and st.site(1) is sites[1] and st.ntargets == 2
    # the Gauss law with the same corr: identical R^-1 on every site
    SiteTargets([site_targets(g, dy=0.01 * s, law_rf="gauss") for s in range(2)]).check()
    with pytest.raises(ValueError, match="distinct"):
        SiteTargets(sites, names=["A", "A", "C"])


def _rejects(sites, match):
    with pytest.raises(ValueError, match=match):
        SiteTargets(sites).check()


def test_mismatches_are_rejected():
    g = golden("chain_golden.npz")
    a = site_targets(g)
    # x one ulp apart
    b = site_targets(g)
    b.targets[0].obsdata.x = np.nextafter(np.asarray(g["xsw"], dtype=float), np.inf)
    _rejects([a, b], "x differs")
    _rejects([a, site_targets(g, p=6.5)], "receiver-function parameters")
    _rejects([a, site_targets(g, mode=2)], "dispersion parameters")
    _rejects([a, site_targets(g, law_rf="nocorr")], "noise law")
    _rejects([site_targets(g, law_rf="gauss", corr=0.9), site_targets(g, law_rf="gauss", corr=0.8)], "R\\^-1")
    # a user plugin
    c = site_targets(g)

    class Fwd(object):
        def run_model(self, h, vp, vs, **kw):
            return g["xsw"], g["ysw"]
    c.targets[0].update_plugin(Fwd())
    _rejects([a, c], "user plugin")
    # another number / class of targets
    _rejects([a, bh.JointTarget([a.targets[0]])], "targets")
    d = site_targets(g)
    d.targets[1] = bh.SReceiverFunction(g["xrf"], g["yrf"])
    d.targets[1].set_noise_law("exp")
    _rejects([a, d], "SReceiverFunction")


@pytest.mark.parametrize("C,nsites,depth", [(1, 1, 1), (4, 3, 1), (4, 3, 3), (8, 64, 2), (5, 2, 7)])
def test_window_column_site_map(C, nsites, depth):
    """node j of chain c of all nsites*C chains sits in column j*(nsites*C) + c; chain c belongs to site c // C"""
    N = (1 << depth) - 1
    ld = nsites * C * N
    want = np.empty(ld, dtype=np.int32)
    for j in range(N):
        for s in range(nsites):
            for c in range(C):
                want[j * nsites * C + s * C + c] = s
    got = window_site_map(C, nsites, ld)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    # the first B = nsites*C*(2^w - 1) entries serve a shorter window w
    for w in range(1, depth + 1):
        B = nsites * C * ((1 << w) - 1)
        assert np.array_equal(got[:B], window_site_map(C, nsites, B))


def test_library_exports_the_site_header():
    from bayhunter_amd import engine as E
    txt = open(os.path.join(REPO, "include", "bh_engine_sites.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decl = sorted(set(re.findall(r"\b(bh_[a-z_]+)\s*\(", txt)))
    assert decl == ["bh_evaluate_sites", "bh_sites_set"]
    assert sorted(E.SITE_SYMBOLS) == decl
    assert not set(decl) & set(E.EXPORTED_SYMBOLS) and not set(decl) & set(E.DEBUG_SYMBOLS)
    lib = ctypes.CDLL(E.LIB_PATH)
    for name in decl:
        assert hasattr(lib, name), "missing export %s" % name


class _RecordingEngine(object):
    """what SiteTargets._register asks of an engine, recorded"""

    def __init__(self):
        self._owner = None
        self.calls = []

    def set_targets(self, descs):
        self.calls.append(("targets", len(descs)))

    def set_sites(self, yobs, yerr=None):
        self.calls.append(("sites", yobs.copy()))


def test_registration_is_checked_once_and_repeated_only_on_change(monkeypatch):
    g = golden("chain_golden.npz")
    eng = _RecordingEngine()
    st = SiteTargets([site_targets(g, dy=0.01 * s) for s in range(3)], engine=eng)
    checks = []
    real = st.check
    monkeypatch.setattr(st, "check", lambda: checks.append(1) or real())
    st._register()
    st._register()
    assert len(checks) == 1 and [c[0] for c in eng.calls] == ["targets", "sites"]
    eng._owner = object()                   # another caller registered its targets: register again, no new check
    st._register()
    assert len(checks) == 1 and len(eng.calls) == 4 and eng._owner is st
    st.site(2).targets[0].obsdata.y = g["ysw"] + 0.5      # a replaced observation: checked and registered again
    st._register()
    assert len(checks) == 2 and len(eng.calls) == 6
    assert np.array_equal(eng.calls[-1][1][2, :21], g["ysw"] + 0.5)
    b = st.site(1).targets[0]
    b.obsdata.x = np.nextafter(np.asarray(g["xsw"], dtype=float), np.inf)
    with pytest.raises(ValueError, match="x differs"):
        st._register()
