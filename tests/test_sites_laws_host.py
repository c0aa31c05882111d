"""Sites with their own noise law (include/bh_engine_sites_laws.h, SiteTargets(per_site_law=True)), the parts that need no GPU: the
header and the library's export, what SiteTargets accepts and refuses with and without the flag, the law table, the slot
descriptors, the correlation classes and the error table it registers, and the order of its registration calls."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, golden
import bayhunter_amd as bh
from bayhunter_amd import engine as E
from bayhunter_amd.sites import SiteTargets
from test_sites_gauss_host import _RecordingEngineGauss
from test_sites_x_host import X_SETS

RCOND = 1e-5
FLAGS = dict(per_site_x="all", per_site_rf=True, missing=True)
NOCORR, SCALED, EXP, GAUSS = E.LAW_NOCORR, E.LAW_NOCORR_SCALED, E.LAW_EXP, E.LAW_GAUSS
# (law of the dispersion curve, law of the receiver function, its fixed correlation) per site; None: the site lacks the slot
LAWS = [("nocorr", "exp", None), ("nocorr_scalederr", "gauss", 0.92), ("exp", "nocorr_scalederr", None),
        ("nocorr_scalederr", None, None), (None, "gauss", 0.98), ("exp", "gauss", 0.92)]


def test_library_exports_the_laws_header():
    txt = open(os.path.join(REPO, "include", "bh_engine_sites_laws.h")).read()
    assert '#include "bh_engine_sites_gauss.h"' in txt
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decl = sorted(set(re.findall(r"\b(bh_[a-z_]+)\s*\(", txt)))
    assert decl == ["bh_sites_set_laws"]
    assert sorted(E.SITE_LAWS_SYMBOLS) == decl
    for other in (E.EXPORTED_SYMBOLS, E.DEBUG_SYMBOLS, E.SITE_SYMBOLS, E.SITE_RF_SYMBOLS, E.SITE_X_SYMBOLS, E.SITE_X_ALL_SYMBOLS,
                  E.SITE_MISSING_SYMBOLS, E.SITE_GAUSS_SYMBOLS, E.SITE_RF_AXIS_SYMBOLS, E.SITE_PRIORS_SYMBOLS, E.POSTERIOR_SYMBOLS):
        assert not set(decl) & set(other)
    lib = ctypes.CDLL(E.LIB_PATH)
    assert hasattr(lib, "bh_sites_set_laws"), "missing export"
    for hdr in sorted(os.listdir(os.path.join(REPO, "include"))):    # declared in the new header only
        if hdr == "bh_engine_sites_laws.h":
            continue
        other = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", hdr)).read(), flags=re.S)
        assert not re.search(r"\bbh_sites_set_laws\b", other), hdr
    lib.bh_abi_version.restype = ctypes.c_int
    assert lib.bh_abi_version() == 10                                # extension headers are outside the contract


def row_of(g, s, laws=LAWS):
    """site s: [Rayleigh phase at its own periods, P receiver function], both WITH error bars, under the laws of laws[s]"""
    swd, rf, corr = laws[s]
    x = np.asarray(X_SETS[s % len(X_SETS)], dtype=float)
    t1 = t2 = None
    if swd is not None:
        t1 = bh.RayleighDispersionPhase(x, 3.4 + 0.01 * x + 0.01 * s, yerr=0.01 + 0.001 * np.arange(x.size) + 0.002 * s)
        t1.set_noise_law(swd)
    if rf is not None:
        n = np.size(g["xrf"])
        t2 = bh.PReceiverFunction(g["xrf"], g["yrf"] * (1.0 + 0.01 * s), yerr=0.02 + 0.0005 * np.arange(n) + 0.001 * s)
        t2.moddata.plugin.set_modelparams(gauss=1.0, p=6.4)
        if rf == "gauss":
            t2.set_noise_law("gauss", corr=corr, rcond=RCOND)
        else:
            t2.set_noise_law(rf)
    return [t1, t2]


def test_the_flag_needs_missing():
    g = golden("chain_golden.npz")
    rows = [row_of(g, s) for s in (0, 1)]
    with pytest.raises(ValueError, match=r"per_site_law=True needs missing=True \(the table of counts it extends\)"):
        SiteTargets(rows, per_site_x="all", per_site_law=True)
    with pytest.raises(ValueError, match="per_site_law=True needs missing=True"):
        SiteTargets(rows, per_site_law=True)
    st = SiteTargets(rows, per_site_law=True, **FLAGS)
    assert st.per_site_law and st.per_site_corr                      # the flag switches the class table on
    assert not SiteTargets(rows, **FLAGS).per_site_law


def test_differing_laws_pass_with_the_flag_and_raise_the_existing_message_without():
    g = golden("chain_golden.npz")
    rows = [row_of(g, s) for s in range(6)]
    SiteTargets(rows, per_site_law=True, **FLAGS).check()
    with pytest.raises(ValueError, match="noise law 'nocorr_scalederr', site 0's 'nocorr'"):
        SiteTargets(rows, **FLAGS).check()
    with pytest.raises(ValueError, match="noise law 'exp', site 0's 'gauss'"):
        SiteTargets([row_of(g, s, [("nocorr", "gauss", 0.9), ("nocorr", "exp", None)]) for s in range(2)], per_site_corr=True, **FLAGS).check()
    # with the flag the other checks stay: a Gauss matrix of another shape among the Gauss sites, another plugin parameter
    bad = row_of(g, 5)
    bad[1].valuation.corr_inv = bad[1].valuation.corr_inv[:60, :60]
    with pytest.raises(ValueError, match="corr_inv has shape|shape"):
        SiteTargets([row_of(g, 0), row_of(g, 1), bad], per_site_law=True, **FLAGS).check()
    other = row_of(g, 2)
    other[1].moddata.plugin.set_modelparams(gauss=2.0)
    with pytest.raises(ValueError, match="receiver-function parameters"):
        SiteTargets([row_of(g, 0), other], per_site_law=True, **FLAGS).check()


def test_the_law_table():
    g = golden("chain_golden.npz")
    st = SiteTargets([row_of(g, s) for s in range(6)], per_site_law=True, **FLAGS)
    law = st.site_law_arrays()
    assert law.shape == (6, 2) and law.dtype == np.int32
    # slot 0's descriptor: site 0's (nocorr, no Gauss site); slot 1's: site 1's (the first Gauss site) -- a lacking site gets them
    assert np.array_equal(law, [[NOCORR, EXP], [SCALED, GAUSS], [EXP, SCALED], [SCALED, GAUSS], [NOCORR, GAUSS], [EXP, GAUSS]])
    assert np.array_equal(st.present, [[1, 1], [1, 1], [1, 1], [1, 0], [0, 1], [1, 1]])


def test_the_slot_descriptor_is_the_first_gauss_sites():
    g = golden("chain_golden.npz")
    laws = [("nocorr", "exp", None), ("exp", "nocorr", None), ("nocorr", None, None), ("exp", "gauss", 0.94)]
    rows = [row_of(g, s, laws) for s in range(4)]
    st = SiteTargets(rows, per_site_law=True, **FLAGS)
    assert st.targets[1] is rows[3][1] and st.targets[0] is rows[0][0]        # a later site is the only Gauss one
    descs = st._capacity_descs()
    assert descs[1]["law"] == GAUSS and descs[0]["law"] == NOCORR
    assert np.asarray(descs[1]["rinv"]).tobytes() == np.ascontiguousarray(rows[3][1].valuation.corr_inv).tobytes()
    # without the flag (one law per slot): the first site that has it, as before
    same = [row_of(g, s, [("nocorr", "exp", None)] * 3) for s in range(3)]
    assert SiteTargets(same, **FLAGS).targets[1] is same[0][1]
    assert SiteTargets(same, per_site_law=True, **FLAGS).targets[1] is same[0][1]


def test_the_classes_skip_the_sites_under_another_law():
    g = golden("chain_golden.npz")
    rows = [row_of(g, s) for s in range(6)]
    st = SiteTargets(rows, per_site_law=True, **FLAGS)
    tables = st.gauss_class_arrays()
    assert sorted(tables) == [1]
    class_of, rinv, logdet = tables[1]
    # site 0: exp, site 2: scaled, site 3: lacks the slot; the classes are numbered by their first Gauss site (0.92, then 0.98)
    assert class_of.dtype == np.int32 and np.array_equal(class_of, [-1, 0, -1, -1, 1, 0])
    assert rinv.shape[0] == 2 and logdet.shape == (2,)
    assert rinv[0].tobytes() == np.ascontiguousarray(rows[1][1].valuation.corr_inv).tobytes()
    assert rinv[1].tobytes() == np.ascontiguousarray(rows[4][1].valuation.corr_inv).tobytes()


def test_the_error_table_holds_yerr_exactly_in_the_cells_under_the_scaled_law():
    g = golden("chain_golden.npz")
    rows = [row_of(g, s) for s in range(6)]
    st = SiteTargets(rows, per_site_law=True, **FLAGS)
    n, x, yobs, yerr = st.site_x_arrays()
    law = st.site_law_arrays()
    cap = n.max(axis=0)
    off = [0, cap[0]]
    assert yerr is not None and yerr.shape == (6, cap.sum())
    for s in range(6):
        for i in range(2):
            cell = yerr[s, off[i]:off[i] + cap[i]]
            if n[s, i] and law[s, i] == SCALED:
                assert np.array_equal(cell[:n[s, i]], np.asarray(rows[s][i].obsdata.yerr, dtype=float)), (s, i)
                assert np.all(cell[n[s, i]:] == 1.0)
            else:                                                    # every other cell: the placeholder, though every target HAS errors
                assert np.all(cell == 1.0), (s, i)
    # no cell under the scaled law: no table
    plain = [row_of(g, s, [("nocorr", "exp", None), ("exp", "gauss", 0.9)]) for s in range(2)]
    assert SiteTargets(plain, per_site_law=True, **FLAGS).site_x_arrays()[3] is None


class _RecordingEngineLaws(_RecordingEngineGauss):
    def set_sites_laws(self, law, yerr=None):
        self.calls.append(("sites_laws", law.copy(), None if yerr is None else yerr.copy()))


def test_registration_order_count_table_rf_tables_laws_classes():
    g = golden("chain_golden.npz")
    eng = _RecordingEngineLaws()
    st = SiteTargets([row_of(g, s) for s in range(6)], engine=eng, per_site_law=True, **FLAGS)
    st._register()
    st._register()
    assert [c[0] for c in eng.calls] == ["targets", "sites_missing_gauss", "sites_rf", "sites_laws", "sites_gauss"]
    assert np.array_equal(eng.calls[3][1], st.site_law_arrays()) and eng.calls[3][2].shape == st.site_x_arrays()[3].shape
    assert [d["law"] for d in eng.calls[0][1]] == [NOCORR, GAUSS]
    assert np.array_equal(eng.calls[4][2], [-1, 0, -1, -1, 1, 0])
    # without the flag: the entry points as before, no law table
    eng2 = _RecordingEngineLaws()
    same = [row_of(g, s, [("nocorr", "gauss", 0.9)] * 2) for s in range(2)]
    SiteTargets(same, engine=eng2, per_site_corr=True, **FLAGS)._register()
    assert [c[0] for c in eng2.calls] == ["targets", "sites_missing_gauss", "sites_rf", "sites_gauss"]


def test_engine_method_passes_the_arrays_to_the_new_entry_point():
    class Lib(object):
        def __init__(self):
            self.calls = []

        def bh_sites_set_laws(self, *a):
            self.calls.append(("laws", a[1], a[3] is not None and a[3].value is not None))
            return 0

    eng = E.Engine.__new__(E.Engine)
    eng._L, eng._h, eng.ldy, eng.ntargets = Lib(), None, 5, 2
    eng.set_sites_laws([[0, 2], [1, 3], [2, 0]], np.ones((3, 5)))
    eng.set_sites_laws(np.zeros((3, 2)))
    assert eng._L.calls == [("laws", 3, True), ("laws", 3, False)]
    with pytest.raises(ValueError, match="law must have shape"):
        eng.set_sites_laws(np.zeros((3, 3)))
    with pytest.raises(ValueError, match="yerr must have shape"):
        eng.set_sites_laws(np.zeros((3, 2)), np.ones((3, 4)))
