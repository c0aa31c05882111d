"""Sites with their own receiver-function time axis and Gauss filter (include/bh_engine_sites_rf_axis.h,
SiteTargets(per_site_rf="all")), the parts that need no GPU: the header and the library's exports, what SiteTargets accepts and
refuses with and without the flag, the tables it registers (axis records, capacity descriptors, padded correlation classes) and
their order."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
import bayhunter_amd as bh
from bayhunter_amd import engine as E
from bayhunter_amd.sites import SiteTargets
from test_sites_x_host import _RecordingEngine

PER = np.linspace(3.0, 40.0, 12)
# (samples, rate Hz, shift s, gauss): the transform lengths follow as 128, 256, 512
AXES = [(64, 5.0, 0.0, 2.5), (65, 10.0, 5.0, 1.0), (201, 5.0, 5.0, 2.5)]
NSAMP = [128, 256, 512]


def rf_target(n, fsamp, tshift, gauss, p=6.4, cls=None, law="exp", corr=None, seed=0):
    x = np.arange(n) / fsamp - tshift
    t = (cls or bh.PReceiverFunction)(x, np.random.RandomState(seed).normal(0, 0.05, n))
    t.moddata.plugin.set_modelparams(gauss=gauss, p=p)
    if law == "gauss":
        t.set_noise_law("gauss", corr=corr, rcond=None)
    else:
        t.set_noise_law(law)
    return t


def swd_target(seed=0):
    t = bh.RayleighDispersionPhase(PER, 3.4 + 0.01 * PER + 0.01 * seed)
    t.set_noise_law("nocorr")
    return t


def sites(axes=AXES, **kw):
    return [bh.JointTarget([swd_target(s), rf_target(*a, p=5.5 + s, seed=s, **kw)]) for s, a in enumerate(axes)]


class _Recorder(_RecordingEngine):
    def set_sites_axes(self, n, x, yobs, yerr=None):
        self.calls.append(("sites_axes", n.copy(), x.copy(), yobs.copy(), None if yerr is None else yerr.copy()))

    def set_sites_rf_axis(self, nsamp, fsamp, tshift, gauss):
        self.calls.append(("sites_rf_axis", nsamp.copy(), fsamp.copy(), tshift.copy(), gauss.copy()))

    def set_sites_gauss(self, target, class_of, rinv, logdet_r):
        self.calls.append(("sites_gauss", int(target), class_of.copy(), rinv.copy(), logdet_r.copy()))


def test_library_exports_the_axis_header():
    txt = open(os.path.join(REPO, "include", "bh_engine_sites_rf_axis.h")).read()
    assert '#include "bh_engine_sites_rf.h"' in txt and '#include "bh_engine_sites_gauss.h"' in txt
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decl = sorted(set(re.findall(r"\b(bh_[a-z_]+)\s*\(", txt)))
    assert decl == ["bh_sites_set_axes", "bh_sites_set_rf_axis"]
    assert sorted(E.SITE_RF_AXIS_SYMBOLS) == decl
    for other in (E.EXPORTED_SYMBOLS, E.DEBUG_SYMBOLS, E.SITE_SYMBOLS, E.SITE_RF_SYMBOLS, E.SITE_X_SYMBOLS, E.SITE_X_ALL_SYMBOLS,
                  E.SITE_MISSING_SYMBOLS, E.SITE_GAUSS_SYMBOLS, E.SITE_PRIORS_SYMBOLS, E.POSTERIOR_SYMBOLS):
        assert not set(decl) & set(other)
    lib = ctypes.CDLL(E.LIB_PATH)
    for name in decl:
        assert hasattr(lib, name), "missing export %s" % name
    for hdr in sorted(os.listdir(os.path.join(REPO, "include"))):          # declared in the new header only
        if hdr == "bh_engine_sites_rf_axis.h":
            continue
        other = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", hdr)).read(), flags=re.S)
        assert not any(re.search(r"\b%s\b" % name, other) for name in decl), hdr
    lib.bh_abi_version.restype = ctypes.c_int
    assert lib.bh_abi_version() == 10                                       # extension headers are outside the contract
    # the header of the shared-axis table no longer calls the axis shared "always"
    assert "always" not in open(os.path.join(REPO, "include", "bh_engine_sites_rf.h")).read()


def test_axes_that_differ_are_refused_without_the_flag_and_register_with_it():
    for kw in (dict(), dict(per_site_rf=True), dict(per_site_x="all", per_site_rf=True)):
        with pytest.raises(ValueError, match=r"x differs from site 0's \(sites share x bit for bit\)"):
            SiteTargets(sites(), **kw).check()
    eng = _Recorder()
    st = SiteTargets(sites(), engine=eng, per_site_x="all", per_site_rf="all")
    st.check()
    assert st.per_site_rf == "all"
    st._register()
    st._register()
    assert [c[0] for c in eng.calls] == ["targets", "sites_axes", "sites_rf", "sites_rf_axis"]
    d = eng.calls[0][1][1]
    assert d["kind"] == E.TARGET_RF and d["n"] == 201 and d["nsamp"] == 512 and np.size(d["yobs"]) == 201
    n, x, yobs, yerr = eng.calls[1][1:]
    assert np.array_equal(n, [[12, 64], [12, 65], [12, 201]]) and yobs.shape == (3, 12 + 201) and yerr is None
    for s, jt in enumerate(st._sites):
        k = n[s, 1]
        assert np.array_equal(yobs[s, 12:12 + k], jt.targets[1].obsdata.y) and np.all(yobs[s, 12 + k:] == 0.0)
        assert np.array_equal(x[s, 12:12 + k], jt.targets[1].obsdata.x)
    assert np.array_equal(eng.calls[2][1][:, 1], [5.5, 6.5, 7.5])


def test_axis_arrays():
    st = SiteTargets(sites(), per_site_x="all", per_site_rf="all")
    nsamp, fsamp, tshift, gauss = st.site_rf_axis_arrays()
    assert nsamp.dtype == np.int32 and nsamp.shape == (3, 2)
    assert np.array_equal(nsamp[:, 1], NSAMP)
    assert np.array_equal(fsamp[:, 1], [a[1] for a in AXES]) and np.array_equal(tshift[:, 1], [a[2] for a in AXES])
    assert np.array_equal(gauss[:, 1], [a[3] for a in AXES])
    # the columns of other targets and of slots a site lacks: placeholders the engine never reads
    assert np.all(nsamp[:, 0] == 4) and np.all(fsamp[:, 0] == 1.0) and np.all(tshift[:, 0] == 0.0) and np.all(gauss[:, 0] == 1.0)
    rows = [[swd_target(0), rf_target(*AXES[0])], [swd_target(1), None], [None, rf_target(*AXES[2])]]
    m = SiteTargets(rows, per_site_x="all", per_site_rf="all", missing=True)
    m.check()
    nsamp, fsamp, tshift, gauss = m.site_rf_axis_arrays()
    assert np.array_equal(nsamp[:, 1], [128, 4, 512]) and np.array_equal(gauss[:, 1], [2.5, 1.0, 2.5])
    assert np.array_equal(m._counts(), [[12, 64], [12, 0], [0, 201]])
    assert m._capacity_descs()[1]["nsamp"] == 512


def test_padded_correlation_classes():
    axes = [(40, 5.0, 0.0, 1.0), (60, 5.0, 2.0, 2.5), (64, 10.0, 2.0, 2.5), (60, 5.0, 1.0, 1.0)]
    corr = [0.90, 0.94, 0.98, 0.94]
    jts = [bh.JointTarget([swd_target(s), rf_target(*a, law="gauss", corr=corr[s], seed=s)]) for s, a in enumerate(axes)]
    eng = _Recorder()
    st = SiteTargets(jts, engine=eng, per_site_x="all", per_site_rf="all", per_site_corr=True)
    st._register()
    assert [c[0] for c in eng.calls] == ["targets", "sites_axes", "sites_rf", "sites_rf_axis", "sites_gauss"]   # the classes last
    d = eng.calls[0][1][1]
    assert d["n"] == 64 and d["rinv"].shape == (64, 64)                      # a placeholder of the capacity
    slot, class_of, rinv, logdet = eng.calls[-1][1:]
    assert slot == 1 and np.array_equal(class_of, [0, 1, 2, 1])              # sites 1 and 3: same bits, same size
    assert rinv.shape == (3, 64, 64)
    for c, s in enumerate((0, 1, 2)):
        v, k = jts[s].targets[1].valuation, axes[s][0]
        assert np.array_equal(rinv[c, :k, :k], v.corr_inv) and np.all(rinv[c, k:, :] == 0.0) and np.all(rinv[c, :, k:] == 0.0)
        assert logdet[c] == float(v.logcorr_det)
    # the same correlation at another sample count is another class: (bits, n)
    two = [bh.JointTarget([rf_target(4, 5.0, 0.0, 1.0, law="gauss", corr=0.5)]), bh.JointTarget([rf_target(6, 5.0, 0.0, 1.0, law="gauss", corr=0.5)])]
    assert np.array_equal(SiteTargets(two, per_site_x="all", per_site_rf="all", per_site_corr=True).gauss_class_arrays()[0][0], [0, 1])
    # counts that differ under the Gauss law need the class table
    with pytest.raises(ValueError, match="Gauss law"):
        SiteTargets(jts, per_site_x="all", per_site_rf="all").check()


def test_refusals():
    for psx in (False, True):
        with pytest.raises(ValueError, match="per_site_rf=\"all\" needs per_site_x=\"all\""):
            SiteTargets(sites(), per_site_x=psx, per_site_rf="all")
    with pytest.raises(ValueError, match="per_site_rf is False, True or \"all\""):
        SiteTargets(sites(), per_site_x="all", per_site_rf="axis")
    A = dict(per_site_x="all", per_site_rf="all")
    # the wave type stays a property of the slot
    jts = sites()
    jts[1] = bh.JointTarget([swd_target(1), rf_target(*AXES[1], cls=bh.SReceiverFunction)])
    with pytest.raises(ValueError, match="is a SReceiverFunction, site 0's is a PReceiverFunction"):
        SiteTargets(jts, **A).check()
    jts = sites()
    jts[2].targets[1].moddata.plugin.set_modelparams(wtype="SV")
    with pytest.raises(ValueError, match="receiver-function parameters"):
        SiteTargets(jts, **A).check()
    # ... and so does the law
    jts = sites()
    jts[1].targets[1].set_noise_law("nocorr")
    with pytest.raises(ValueError, match="noise law 'nocorr', site 0's 'exp'"):
        SiteTargets(jts, **A).check()
    # more than 16384 points: 8193 samples need a transform of 16384 * 2
    with pytest.raises(ValueError, match="a transform of 32768 points; a site has at most 16384"):
        SiteTargets(sites(AXES[:2] + [(8193, 20.0, 5.0, 2.5)]), **A).check()
    SiteTargets(sites(AXES[:2] + [(8192, 20.0, 5.0, 2.5)]), **A).check()
    # True keeps its meaning: p and nsv only
    with pytest.raises(ValueError, match="receiver-function parameters"):
        same_x = [bh.JointTarget([rf_target(64, 5.0, 0.0, g)]) for g in (1.0, 2.5)]
        SiteTargets(same_x, per_site_x="all", per_site_rf=True).check()
