"""Sites with their own Gauss-law noise correlation (include/bh_engine_sites_gauss.h, SiteTargets(per_site_corr=True)), the parts
that need no GPU: the header and the library's exports, what SiteTargets accepts and refuses with and without the flag, the
correlation classes it registers and the order of its registration calls."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, golden
import bayhunter_amd as bh
from bayhunter_amd.sites import SiteTargets
from test_sites_missing_host import _RecordingEngineMissing
from test_sites_x_host import X_FULL, X_SETS

CORR = [0.90, 0.94, 0.94, 0.98]
RCOND = 1e-5


def test_library_exports_the_gauss_header():
    from bayhunter_amd import engine as E
    txt = open(os.path.join(REPO, "include", "bh_engine_sites_gauss.h")).read()
    assert '#include "bh_engine_sites_missing.h"' in txt
    assert re.search(r"#define\s+BH_SITES_GAUSS_MAXBYTES\b", txt)
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decl = sorted(set(re.findall(r"\b(bh_[a-z_]+)\s*\(", txt)))
    assert decl == ["bh_sites_set_gauss", "bh_sites_set_missing_gauss"]
    assert sorted(E.SITE_GAUSS_SYMBOLS) == decl
    for other in (E.EXPORTED_SYMBOLS, E.DEBUG_SYMBOLS, E.SITE_SYMBOLS, E.SITE_RF_SYMBOLS, E.SITE_X_SYMBOLS, E.SITE_X_ALL_SYMBOLS,
                  E.SITE_MISSING_SYMBOLS, E.SITE_PRIORS_SYMBOLS, E.POSTERIOR_SYMBOLS):
        assert not set(decl) & set(other)
    lib = ctypes.CDLL(E.LIB_PATH)
    for name in decl:
        assert hasattr(lib, name), "missing export %s" % name
    for hdr in sorted(os.listdir(os.path.join(REPO, "include"))):    # declared in the new header only
        if hdr == "bh_engine_sites_gauss.h":
            continue
        other = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", hdr)).read(), flags=re.S)
        assert not any(re.search(r"\b%s\b" % name, other) for name in decl), hdr
    lib.bh_abi_version.restype = ctypes.c_int
    assert lib.bh_abi_version() == 10                                # extension headers are outside the contract


def slots_of(g, x, corr, dy=0.0, have="11", nrf=None, rf_law="gauss"):
    """[Rayleigh phase, P receiver function with the noise correlation fixed at `corr`] of a site, None where `have` says 0"""
    x = np.asarray(x, dtype=float)
    t1 = bh.RayleighDispersionPhase(x, 3.4 + 0.01 * x + dy)
    t1.set_noise_law("nocorr")
    xrf, yrf = g["xrf"][:nrf], g["yrf"][:nrf]
    t2 = bh.PReceiverFunction(xrf, yrf * (1.0 + dy))
    t2.moddata.plugin.set_modelparams(gauss=1.0, p=6.4)
    if rf_law == "gauss":
        t2.set_noise_law("gauss", corr=corr, rcond=RCOND)
    else:
        t2.set_noise_law(rf_law)
    return [t if c == "1" else None for t, c in zip((t1, t2), have)]


def test_per_site_corr_accepts_differing_correlations_and_builds_the_classes():
    g = golden("chain_golden.npz")
    rows = [slots_of(g, X_FULL, CORR[s], 0.01 * s) for s in range(4)]
    st = SiteTargets(rows, per_site_corr=True)
    st.check()
    assert st.per_site_corr and not SiteTargets(rows).per_site_corr
    tables = st.gauss_class_arrays()
    assert sorted(tables) == [1]                                     # one table, for the Gauss-law target
    class_of, rinv, logdet = tables[1]
    n = np.size(g["xrf"])
    assert class_of.dtype == np.int32 and np.array_equal(class_of, [0, 1, 1, 2])
    assert rinv.shape == (3, n, n) and rinv.dtype == np.float64 and logdet.shape == (3,)
    for s in range(4):                                               # each matrix: what init_covariance_gauss left at that site
        v = rows[s][1].valuation
        assert rinv[class_of[s]].tobytes() == np.ascontiguousarray(v.corr_inv, dtype=np.float64).tobytes()
        assert logdet[class_of[s]].tobytes() == np.float64(v.logcorr_det).tobytes()
    assert rinv[0].tobytes() != rinv[1].tobytes() != rinv[2].tobytes()
    # sites that all fix one value: one class
    one = SiteTargets([slots_of(g, X_FULL, 0.98, 0.01 * s) for s in range(3)], per_site_corr=True).gauss_class_arrays()[1]
    assert np.array_equal(one[0], [0, 0, 0]) and one[1].shape == (1, n, n)


def test_without_the_flag_the_same_sites_raise_the_existing_message():
    g = golden("chain_golden.npz")
    rows = [slots_of(g, X_FULL, CORR[s], 0.01 * s) for s in range(4)]
    with pytest.raises(ValueError, match=r"Gauss law with another R\^-1 / ln\|R\| than site 0's \(sites share corr\)"):
        SiteTargets(rows).check()
    M = dict(per_site_x="all", missing=True)
    with pytest.raises(ValueError, match="Gauss law on a slot that some site lacks"):
        SiteTargets([slots_of(g, X_FULL, 0.9), slots_of(g, X_FULL, 0.9, have="10")], **M).check()
    # the law mismatch stays refused in every mode
    with pytest.raises(ValueError, match="noise law 'exp', site 0's 'gauss'"):
        SiteTargets([slots_of(g, X_FULL, 0.9), slots_of(g, X_FULL, 0.9, rf_law="exp")], per_site_corr=True).check()


def test_missing_gauss_slot_gets_class_minus_one_and_the_refusals_that_stay():
    g = golden("chain_golden.npz")
    M = dict(per_site_x="all", missing=True, per_site_corr=True)
    have = ["11", "10", "11", "01"]
    rows = [slots_of(g, X_SETS[s], CORR[s], 0.01 * s, have[s]) for s in range(4)]
    st = SiteTargets(rows, **M)
    st.check()
    class_of, rinv, logdet = st.gauss_class_arrays()[1]
    assert np.array_equal(class_of, [0, -1, 1, 2]) and rinv.shape[0] == 3
    assert rinv[1].tobytes() == np.ascontiguousarray(rows[2][1].valuation.corr_inv).tobytes()
    # a differing shape (another sample count) is refused: the sample count stays shared
    # (a receiver function of another length differs in x first; a matrix that does not fit its own samples is Target.law()'s)
    short = slots_of(g, X_FULL, 0.94, nrf=60)
    assert short[1].valuation.corr_inv.shape == (60, 60)
    with pytest.raises(ValueError, match="x differs from site 0's"):
        SiteTargets([rows[0], short], **M).check()
    full = slots_of(g, X_FULL, 0.94)
    full[1].valuation.corr_inv = short[1].valuation.corr_inv
    with pytest.raises(ValueError, match="shape"):
        SiteTargets([rows[0], full], **M).check()
    # a Gauss-law dispersion target with periods per site is still refused
    def gauss_swd(x, corr):
        row = slots_of(g, x, 0.9)
        row[0].set_noise_law("gauss", corr=corr, rcond=RCOND)
        return row
    with pytest.raises(ValueError, match="Gauss law on a dispersion target with periods per site"):
        SiteTargets([gauss_swd(X_SETS[0], 0.5), gauss_swd(X_SETS[1], 0.6)], **M).check()


class _RecordingEngineGauss(_RecordingEngineMissing):
    def set_sites_missing_gauss(self, n, x, yobs, yerr=None):
        self.calls.append(("sites_missing_gauss", n.copy()))

    def set_sites_gauss(self, target, class_of, rinv, logdet_r):
        self.calls.append(("sites_gauss", int(target), class_of.copy(), rinv.copy(), logdet_r.copy()))


def test_registration_order_the_classes_come_last():
    g = golden("chain_golden.npz")
    eng = _RecordingEngineGauss()
    rows = [slots_of(g, X_FULL, CORR[s], 0.01 * s) for s in range(4)]
    st = SiteTargets(rows, engine=eng, per_site_corr=True)
    st._register()
    st._register()
    assert [c[0] for c in eng.calls] == ["targets", "sites", "sites_gauss"]
    assert eng.calls[2][1] == 1 and np.array_equal(eng.calls[2][2], [0, 1, 1, 2]) and eng.calls[2][3].shape[0] == 3
    # the descriptor's matrix: site 0's
    assert np.asarray(eng.calls[0][1][1]["rinv"]).tobytes() == np.ascontiguousarray(rows[0][1].valuation.corr_inv).tobytes()
    eng2 = _RecordingEngineGauss()
    have = ["11", "10", "11", "01"]
    rows2 = [slots_of(g, X_SETS[s], CORR[s], 0.01 * s, have[s]) for s in range(4)]
    SiteTargets(rows2, engine=eng2, per_site_x="all", missing=True, per_site_corr=True)._register()
    assert [c[0] for c in eng2.calls] == ["targets", "sites_missing_gauss", "sites_rf", "sites_gauss"]
    assert np.array_equal(eng2.calls[1][1][:, 1] == 0, [False, True, False, False])
    assert np.array_equal(eng2.calls[3][2], [0, -1, 1, 2])
    # without the flag: the entry points as before, no class table
    eng3 = _RecordingEngineGauss()
    SiteTargets([slots_of(g, X_FULL, 0.9, 0.01 * s) for s in range(2)], engine=eng3)._register()
    assert [c[0] for c in eng3.calls] == ["targets", "sites"]


def test_engine_methods_pass_the_arrays_to_the_new_entry_points():
    from bayhunter_amd import engine as E

    class Lib(object):
        def __init__(self):
            self.calls = []

        def bh_sites_set_missing_gauss(self, *a):
            self.calls.append(("missing_gauss", a[1]))
            return 0

        def bh_sites_set_gauss(self, *a):
            self.calls.append(("gauss", a[1], a[2], a[3]))
            return 0

    eng = E.Engine.__new__(E.Engine)
    eng._L, eng._h, eng.ldy, eng.ntargets = Lib(), None, 5, 2
    n = np.array([[2, 3], [0, 3], [2, 0]], np.int32)
    eng.set_sites_missing_gauss(n, np.ones((3, 5)), np.zeros((3, 5)))
    eng.set_sites_gauss(1, [0, 1, -1], np.zeros((2, 3, 3)), np.zeros(2))
    assert eng._L.calls == [("missing_gauss", 3), ("gauss", 1, 3, 2)] and eng.nsites == 3
    with pytest.raises(ValueError, match="rinv must have shape"):
        eng.set_sites_gauss(1, [0, 1, -1], np.zeros((2, 3, 4)), np.zeros(2))
    with pytest.raises(ValueError, match="rinv must have shape"):
        eng.set_sites_gauss(1, [0, 1, -1], np.zeros((2, 3, 3)), np.zeros(3))
