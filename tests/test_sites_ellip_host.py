"""The Rayleigh ellipticity with its own periods at every site, or absent at a site (include/bh_engine_sites_ellip.h,
SiteTargets(per_site_ellip=True)), the parts that need no GPU: the header and the library's exports, the pure plan of where such a
target's velocities come from under a count table (bh_plan_ellip_sites) row by row, and what a site set admits, refuses and
registers with the flag -- and that without it every message is what tests/test_ellip_fused_host.py pins."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO
import bayhunter_amd as bh
from bayhunter_amd import engine as E
from bayhunter_amd.sites import SiteTargets
from bayhunter_amd.Targets import LAWS

SWD, RF, USER, ELLIP = 0, 1, 2, 3
RAYLEIGH, LOVE, PHASE, GROUP = 2, 1, 0, 1
X = np.array([2.0, 4.0, 8.0, 12.0, 20.0, 28.0, 33.0])


# ---- header and exports -----------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_two_calls():
    txt = open(os.path.join(REPO, "include", "bh_engine_sites_ellip.h")).read()
    assert '#include "bh_engine_ellip_target.h"' in txt and '#include "bh_engine_sites_missing.h"' in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decl = sorted(set(re.findall(r"\b(bh_[a-z_]+)\s*\(", code)))
    assert decl == ["bh_plan_ellip_sites", "bh_targets_set_ellip_sites"]
    assert re.search(r"int\s+bh_targets_set_ellip_sites\(bh_engine \*e, int t, int own\)", code)
    assert sorted(E.SITE_ELLIP_SYMBOLS) == decl
    for other in (E.EXPORTED_SYMBOLS, E.DEBUG_SYMBOLS, E.SITE_SYMBOLS, E.SITE_X_ALL_SYMBOLS, E.SITE_MISSING_SYMBOLS, E.SWD_ELLIP_SYMBOLS,
                  E.ELLIP_TARGET_SYMBOLS):
        assert not set(decl) & set(other)
    lib = C.CDLL(E.LIB_PATH)
    for name in decl:
        assert hasattr(lib, name), "missing export %s" % name
    for hdr in sorted(os.listdir(os.path.join(REPO, "include"))):    # declared in the new header only; bh_engine.h does not mention them
        if hdr == "bh_engine_sites_ellip.h":
            continue
        other = open(os.path.join(REPO, "include", hdr)).read()
        if hdr != "bh_engine.h":
            other = re.sub(r"/\*.*?\*/", "", other, flags=re.S)
        for name in decl:
            assert name not in other, (hdr, name)
    lib.bh_abi_version.restype = C.c_int
    assert lib.bh_abi_version() == 10
    for word in ("THE RULE PER MODEL", "CAPACITY", "forces the search", "bh_evaluate_batch"):
        assert word in txt
    assert hasattr(E.Engine, "set_target_ellip_sites")


# ---- the pure plan ----------------------------------------------------------------------------------------------------------------
class PlanTarget(C.Structure):   # bh_ellip_plan_target
    _fields_ = [(k, C.c_int32) for k in ("kind", "iwave", "igr", "mode", "flsph", "n", "xid")]


def _lib():
    lib = C.CDLL(E.LIB_PATH)
    lib.bh_plan_ellip_sites.restype = C.c_int
    lib.bh_plan_ellip_sites.argtypes = [C.c_int, C.POINTER(PlanTarget), C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32),
                                        C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    return lib


def plan(targets, sites, own=None):
    """targets: (kind, iwave, igr, mode, flsph) per target; sites: per site a list with every target's periods (None / empty: the site
    lacks it); own: the flag per target (default: every ellipticity target has it).  The tables as SiteTargets.site_x_arrays lays
    them out.  Returns (source per target, searches added)."""
    nt, S = len(targets), len(sites)
    n = np.array([[0 if x is None else len(x) for x in row] for row in sites], dtype=np.int32).reshape(S, nt)
    cap = n.max(axis=0)
    off = np.concatenate([[0], np.cumsum(cap)]).astype(np.int32)
    x = np.zeros((S, max(int(off[-1]), 1)))
    for s, row in enumerate(sites):
        for t, per in enumerate(row):
            if per is not None:
                x[s, off[t]:off[t] + len(per)] = per
    arr = (PlanTarget * 8)()
    for t, (kind, iwave, igr, mode, flsph) in enumerate(targets):
        arr[t] = PlanTarget(kind, iwave, igr, mode, flsph, int(cap[t]), -1)
    flags = np.array([(k[0] == ELLIP) if own is None else own[t] for t, k in enumerate(targets)], dtype=np.int32)
    src = (C.c_int32 * 8)(*([99] * 8))
    offs = np.ascontiguousarray(off[:nt])
    added = _lib().bh_plan_ellip_sites(nt, arr, flags.ctypes.data_as(C.POINTER(C.c_int32)), S, n.ctypes.data_as(C.POINTER(C.c_int32)),
                                       x.ctypes.data_as(C.POINTER(C.c_double)), x.shape[1], offs.ctypes.data_as(C.POINTER(C.c_int32)), src)
    return list(src)[:nt], added


R_PH = (SWD, RAYLEIGH, PHASE, 1, 0)
ELL = (ELLIP, RAYLEIGH, PHASE, 1, 0)
XA, XB, XC3 = X, X[:4] * 1.5, X[2:5]
XA_BIT = XA.copy()
XA_BIT[5] = np.nextafter(XA[5], 100.0)


@pytest.mark.parametrize("targets, sites, own, want", [
    ([R_PH, ELL], [[XA, XA], [XB, XB], [XC3, XC3]], None, ([-2, 0], 0)),          # equal periods at every site that has t
    ([R_PH, ELL], [[XA, XA], [XB, XB], [XA, XA_BIT]], None, ([-2, -1], 1)),        # one differing bit at one site
    ([R_PH, ELL], [[XA, XA], [XB, XB[:3]], [XC3, XC3]], None, ([-2, -1], 1)),      # another count at one site
    ([R_PH, ELL], [[XA, XA], [None, XB], [XC3, XC3]], None, ([-2, -1], 1)),        # a site that has t and lacks j
    ([R_PH, ELL], [[XA, XA], [XB, None], [XC3, XC3]], None, ([-2, 0], 0)),         # a site that has j and lacks t
    ([(SWD, RAYLEIGH, GROUP, 1, 0), ELL], [[XA, XA], [XB, XB]], None, ([-2, -1], 1)),   # a group velocity: skipped
    ([(SWD, LOVE, PHASE, 1, 0), ELL], [[XA, XA], [XB, XB]], None, ([-2, -1], 1)),       # Love
    ([(SWD, RAYLEIGH, PHASE, 2, 0), ELL], [[XA, XA], [XB, XB]], None, ([-2, -1], 1)),   # the first overtone
    ([(SWD, RAYLEIGH, PHASE, 1, 1), ELL], [[XA, XA], [XB, XB]], None, ([-2, -1], 1)),   # flattened
    ([(SWD, LOVE, PHASE, 1, 0), R_PH, ELL], [[XA, XA, XA], [XB, XB, XB]], None, ([-2, -2, 1], 0)),   # ... the first that qualifies
    ([R_PH, R_PH, ELL], [[XB, XA, XA], [XB, XB, XB]], None, ([-2, -2, 1], 0)),     # target 0 differs at site 0, target 1 serves
    ([ELL, ELL], [[XA, XA], [XB, XB]], None, ([-1, -1], 2)),                      # two ellipticities never share with each other
    ([R_PH, ELL, ELL], [[XA, XA, XA], [XB, XB, XB[:2]]], None, ([-2, 0, -1], 1)),  # ... each decided on its own
    ([R_PH, ELL], [[XA, XA], [XA, XA]], [0, 0], ([-2, -1], 1)),                    # an unflagged target under a table: as today
    ([R_PH, ELL, ELL], [[XA, XA, XA], [XB, XB, XB]], [0, 0, 1], ([-2, -1, 0], 1)),
    ([R_PH, (USER, 0, 0, 0, 0)], [[XA, XA], [XB, XB]], [0, 0], ([-2, -2], 0)),
])
def test_plan_shares_a_search_where_every_site_that_has_the_target_allows_it(targets, sites, own, want):
    assert plan(targets, sites, own) == want


def test_plan_refuses_null_arguments_and_a_target_count_out_of_range():
    lib = _lib()
    arr = (PlanTarget * 2)(PlanTarget(SWD, RAYLEIGH, PHASE, 1, 0, 3, -1), PlanTarget(ELLIP, RAYLEIGH, PHASE, 1, 0, 3, -1))
    own, n, off, src = (C.c_int32 * 2)(0, 1), (C.c_int32 * 2)(3, 3), (C.c_int32 * 2)(0, 3), (C.c_int32 * 2)()
    x = (C.c_double * 6)(1, 2, 3, 1, 2, 3)
    assert lib.bh_plan_ellip_sites(2, arr, own, 1, n, x, 6, off, src) == 0 and list(src) == [-2, 0]
    assert lib.bh_plan_ellip_sites(9, arr, own, 1, n, x, 6, off, src) == -1
    assert lib.bh_plan_ellip_sites(-1, arr, own, 1, n, x, 6, off, src) == -1
    assert lib.bh_plan_ellip_sites(2, arr, own, 0, n, x, 6, off, src) == -1
    for k in range(6):
        args = [arr, own, n, x, off, src]
        args[k] = None
        assert lib.bh_plan_ellip_sites(2, args[0], args[1], 1, args[2], args[3], 6, args[4], args[5]) == -1, k
    # a capacity above 60 never serves
    arr[0].n = 61
    assert lib.bh_plan_ellip_sites(2, arr, own, 1, n, x, 6, off, src) == 1 and list(src) == [-2, -1]


def test_the_plan_of_the_fused_call_is_as_it_was():
    """bh_plan_ellip keeps its row "a period table is in force -> a search of its own" """
    from test_ellip_fused_host import plan as plan0, swd, ELL as ELL0
    assert plan0([swd(), ELL0], True) == ([-2, -1], 1) and plan0([swd(), ELL0], False) == ([-2, 0], 0)


# ---- the site set -----------------------------------------------------------------------------------------------------------------
def ell_target(x=X, law="nocorr", yerr=None, **params):
    x = np.asarray(x, dtype=float)
    t = bh.RayleighEllipticity(x, 0.8 + 0.01 * x, yerr=yerr, fused=True)
    t.set_noise_law(law)
    if params:
        t.moddata.plugin.set_modelparams(**params)
    return t


def phase_target(x=X):
    t = bh.RayleighDispersionPhase(x, 3.0 + 0.02 * x)
    t.set_noise_law("nocorr")
    return t


COUNTS = (7, 3, 1, 0)
ELL_X = [X * 1.1, X[1:4] * 0.9, X[3:4], None]


def four_sites(**kw):
    rows = [[phase_target(X[:5 + s % 3]), None if ELL_X[s] is None else ell_target(ELL_X[s])] for s in range(4)]
    return SiteTargets(rows, per_site_x="all", missing=True, per_site_ellip=True, **kw)


def test_flag_needs_the_table_of_every_dispersion_target():
    for flag in (False, True):
        with pytest.raises(ValueError, match=r'per_site_ellip=True needs per_site_x="all"'):
            SiteTargets([[phase_target(), ell_target()]], per_site_x=flag, per_site_ellip=True)


def test_with_the_flag_check_admits_own_periods_own_counts_and_an_absent_slot():
    SiteTargets([[phase_target(), ell_target(X * (1.0 + 0.1 * s))] for s in range(3)], per_site_x="all", per_site_ellip=True).check()
    SiteTargets([[phase_target(), ell_target(X[:7 - 2 * s])] for s in range(3)], per_site_x="all", per_site_ellip=True).check()
    st = four_sites()
    st.check()
    assert st.present.tolist() == [[True, True], [True, True], [True, True], [True, False]]
    four_sites(per_site_law=True).check()
    # without missing=True a None is no site's slot
    with pytest.raises(Exception):
        SiteTargets([[phase_target(), ell_target()], [phase_target(), None]], per_site_x="all", per_site_ellip=True).check()


def test_with_the_flag_check_still_refuses():
    kw = dict(per_site_x="all", per_site_ellip=True)
    with pytest.raises(ValueError, match=r"rellip.*ellipticity parameters \(nsteps, signed, ratio\) \(1, False, 'hv'\)"):
        SiteTargets([[phase_target(), ell_target()], [phase_target(), ell_target(X[:3], nsteps=1)]], **kw).check()
    with pytest.raises(ValueError, match=r"rellip.*ellipticity parameters"):
        SiteTargets([[phase_target(), ell_target()], [phase_target(), ell_target(X[:3], ratio="zh")]], missing=True, **kw).check()
    # the Gauss law, like a dispersion slot's
    g = [ell_target(), ell_target(X[:4])]
    for t in g:
        t.set_noise_law("gauss", corr=0.5)
    with pytest.raises(ValueError, match=r"rellip.*Gauss law on an ellipticity target with periods per site"):
        SiteTargets([[phase_target(), g[0]], [phase_target(), g[1]]], **kw).check()
    # 61 periods (the target itself takes 60 at the most: the site's arrays are replaced afterwards)
    long = ell_target(np.linspace(1.0, 40.0, 60))
    long.obsdata.x = np.linspace(1.0, 40.0, 61)
    long.obsdata.y = np.ones(61)
    with pytest.raises(ValueError, match=r"rellip.*61 periods; a site has 1 to 60 with per_site_ellip"):
        SiteTargets([[phase_target(), ell_target()], [phase_target(), long]], **kw).check()
    bad = X.copy()
    bad[2] = -1.0
    neg = ell_target()
    neg.obsdata.x = bad
    with pytest.raises(ValueError, match=r"rellip.*not finite and positive"):
        SiteTargets([[phase_target(), ell_target()], [phase_target(), neg]], **kw).check()
    with pytest.raises(ValueError, match="a user plugin"):
        u = bh.RayleighEllipticity(X[:3], np.ones(3))
        u.set_noise_law("nocorr")
        SiteTargets([[phase_target(), ell_target()], [phase_target(), u]], **kw).check()


def test_arrays_for_counts_seven_three_one_zero():
    st = four_sites()
    n = st._counts()
    assert n.dtype == np.int32 and n[:, 1].tolist() == list(COUNTS) and n[:, 0].tolist() == [5, 6, 7, 5]
    descs = st._capacity_descs()
    d = descs[1]
    assert d["kind"] == E.TARGET_USER and d["n"] == 7 and d["ellip_sites"] is True and d["nsteps"] == 2
    assert np.array_equal(d["x"], np.ones(7)) and np.array_equal(d["yobs"], np.zeros(7)) and "yerr" not in d
    assert descs[0]["n"] == 7 and "ellip_sites" not in descs[0]
    cnt, x, yobs, yerr = st.site_x_arrays()
    assert np.array_equal(cnt, n) and x.shape == (4, 14) and yerr is None
    for s, per in enumerate(ELL_X):
        k = COUNTS[s]
        if k:
            assert np.array_equal(x[s, 7:7 + k], per) and np.array_equal(yobs[s, 7:7 + k], 0.8 + 0.01 * per)
        assert np.all(x[s, 7 + k:] == 0.0) and np.all(yobs[s, 7 + k:] == 0.0)
    # error bars at one station only (per_site_law): the descriptor's placeholder errors, the table's own
    rows = [[phase_target(), ell_target(X, law="nocorr_scalederr", yerr=0.02 + 0.001 * X)], [phase_target(), ell_target(X[:3])],
            [phase_target(), None]]
    sl = SiteTargets(rows, per_site_x="all", missing=True, per_site_law=True, per_site_ellip=True)
    sl.check()
    d = sl._capacity_descs()[1]
    assert d["ellip_sites"] and np.array_equal(d["yerr"], np.ones(7))
    _, _, _, yerr = sl.site_x_arrays()
    assert np.array_equal(yerr[0, 7:], 0.02 + 0.001 * X) and np.all(yerr[1:] == 1.0)
    assert sl.site_law_arrays()[:2, 1].tolist() == [LAWS["nocorr_scalederr"], LAWS["nocorr"]]
    # without the flag the descriptor is the first site's and carries no key
    plain = SiteTargets([[phase_target(), ell_target()] for _ in range(2)], per_site_x="all")
    d = plain._capacity_descs()[1]
    assert "ellip_sites" not in d and np.array_equal(d["x"], X)


def test_without_the_flag_the_messages_are_unchanged():
    with pytest.raises(ValueError, match=r"rellip.*missing=True does not serve a RayleighEllipticity slot \(every site has the "
                                         r"ellipticity, at shared periods\)"):
        SiteTargets([[phase_target(), ell_target()], [phase_target(), None]], per_site_x="all", missing=True).check()
    other = X.copy()
    other[2] = 9.0
    for flag in (False, True, "all"):
        with pytest.raises(ValueError, match=r"rellip.*x differs from site 0's \(sites share x bit for bit\)"):
            SiteTargets([[phase_target(), ell_target()], [phase_target(), ell_target(other)]], per_site_x=flag).check()
    import test_ellip_fused_host as old
    old.test_site_set_admits_the_fused_slot_and_names_what_it_refuses()
