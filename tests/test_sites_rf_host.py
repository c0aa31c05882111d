"""Receiver-function parameters per site (include/bh_engine_sites_rf.h, SiteTargets(per_site_rf=True)), the parts that need no
GPU: the header and the library's export, what SiteTargets accepts and rejects, and what it registers."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, golden
import bayhunter_amd as bh
from bayhunter_amd.sites import SiteTargets


def rf_site(g, dy=0.0, p=6.4, nsv=None, gauss=1.0, law_rf="exp", sv=False):
    t1 = bh.RayleighDispersionPhase(g["xsw"], g["ysw"] + dy)
    t2 = (bh.SReceiverFunction if sv else bh.PReceiverFunction)(g["xrf"], g["yrf"] * (1.0 + dy))
    t2.moddata.plugin.set_modelparams(gauss=gauss, p=p, nsv=nsv)
    t1.set_noise_law("nocorr")
    t2.set_noise_law(law_rf)
    return bh.JointTarget([t1, t2])


def test_library_exports_the_site_rf_header():
    from bayhunter_amd import engine as E
    txt = open(os.path.join(REPO, "include", "bh_engine_sites_rf.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decl = sorted(set(re.findall(r"\b(bh_[a-z_]+)\s*\(", txt)))
    assert decl == ["bh_sites_set_rf"]
    assert sorted(E.SITE_RF_SYMBOLS) == decl
    for other in (E.EXPORTED_SYMBOLS, E.DEBUG_SYMBOLS, E.SITE_SYMBOLS, E.POSTERIOR_SYMBOLS):
        assert not set(decl) & set(other)
    lib = ctypes.CDLL(E.LIB_PATH)
    for name in decl:
        assert hasattr(lib, name), "missing export %s" % name


def test_per_site_rf_accepts_differing_p_and_nsv():
    g = golden("chain_golden.npz")
    sites = [rf_site(g, 0.01 * s, p=5.5 + s, nsv=(None if s % 2 == 0 else 1.5 + s)) for s in range(4)]
    SiteTargets(sites, per_site_rf=True).check()
    with pytest.raises(ValueError, match="receiver-function parameters"):      # the default still refuses them
        SiteTargets(sites).check()
    with pytest.raises(ValueError, match="receiver-function parameters"):
        SiteTargets([rf_site(g), rf_site(g, nsv=2.0)]).check()
    assert not SiteTargets(sites).per_site_rf


def _rejects(sites, match):
    with pytest.raises(ValueError, match=match):
        SiteTargets(sites, per_site_rf=True).check()


def test_per_site_rf_still_rejects_every_other_mismatch():
    g = golden("chain_golden.npz")
    a = rf_site(g, p=5.5)
    _rejects([a, rf_site(g, p=7.0, gauss=2.5)], "receiver-function parameters")
    b = rf_site(g, p=7.0)
    b.targets[1].moddata.plugin.tshft = a.targets[1].moddata.plugin.tshft + 1.0
    _rejects([a, b], "receiver-function parameters")
    c = rf_site(g, p=7.0)
    c.targets[1].moddata.plugin.nsamp *= 2
    _rejects([a, c], "receiver-function parameters")
    d = rf_site(g, p=7.0)
    d.targets[1].obsdata.x = np.nextafter(np.asarray(g["xrf"], dtype=float), np.inf)
    _rejects([a, d], "x differs")
    _rejects([a, rf_site(g, p=7.0, sv=True)], "SReceiverFunction")
    _rejects([a, rf_site(g, p=7.0, law_rf="nocorr")], "noise law")


class _RecordingEngine(object):
    """what SiteTargets._register asks of an engine, recorded"""

    def __init__(self):
        self._owner = None
        self.calls = []

    def set_targets(self, descs):
        self.calls.append(("targets", [dict(d) for d in descs]))

    def set_sites(self, yobs, yerr=None):
        self.calls.append(("sites", yobs.copy()))

    def set_sites_rf(self, p, nsv):
        self.calls.append(("sites_rf", np.array(p, dtype=float), np.array(nsv, dtype=float)))


def test_registration_passes_each_sites_p_and_nsv():
    g = golden("chain_golden.npz")
    eng = _RecordingEngine()
    P, NSV = (5.5, 6.4, 7.5), (None, 2.0, None)
    st = SiteTargets([rf_site(g, 0.01 * s, p=P[s], nsv=NSV[s]) for s in range(3)], engine=eng, per_site_rf=True)
    st._register()
    st._register()
    assert [c[0] for c in eng.calls] == ["targets", "sites", "sites_rf"]
    _, p, nsv = eng.calls[2]
    assert p.shape == nsv.shape == (3, 2)
    assert np.array_equal(p, [[0.0, 5.5], [0.0, 6.4], [0.0, 7.5]])
    assert np.array_equal(nsv, [[0.0, 0.0], [0.0, 2.0], [0.0, 0.0]])
    assert eng.calls[0][1][1]["p"] == 5.5                     # the descriptor: site 0's
    st.site(2).targets[1].moddata.plugin.set_modelparams(p=8.25)   # one site's p changed: registered again
    st._register()
    assert [c[0] for c in eng.calls[3:]] == ["targets", "sites", "sites_rf"]
    assert eng.calls[-1][1][2, 1] == 8.25 and eng.calls[-1][1][0, 1] == 5.5
    plain = _RecordingEngine()                               # without per_site_rf: no table of p and nsv
    SiteTargets([rf_site(g, 0.01 * s) for s in range(2)], engine=plain)._register()
    assert [c[0] for c in plain.calls] == ["targets", "sites"]
