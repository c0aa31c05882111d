"""The Rayleigh ellipticity as a target of the fused call (include/bh_engine_ellip_target.h), the parts that need no GPU: the header
and the library's exports, the pure plan of where an ellipticity target's velocities come from (bh_plan_ellip) row by row, how
`RayleighEllipticity(fused=True)` describes itself to the engine, and what a site set admits and refuses of it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO
import bayhunter_amd as bh
from bayhunter_amd import engine as E
from bayhunter_amd.sites import SiteTargets

X = np.array([2.0, 4.0, 8.0, 12.0, 20.0])
SWD, RF, USER, ELLIP = 0, 1, 2, 3
RAYLEIGH, LOVE, PHASE, GROUP = 2, 1, 0, 1


def test_header_declares_and_library_exports_the_target_call():
    txt = open(os.path.join(REPO, "include", "bh_engine_ellip_target.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decl = sorted(set(re.findall(r"\b(bh_[a-z_]+)\s*\(", code)))
    assert decl == ["bh_plan_ellip", "bh_targets_set_ellip"]
    assert re.search(r"#define\s+BH_TARGET_ELLIP\s+3\b", code)
    assert re.search(r"int\s+bh_targets_set_ellip\(bh_engine \*e, int t, int K, const double \*periods, int nsteps, int is_signed, int zh\)", code)
    assert sorted(E.ELLIP_TARGET_SYMBOLS) == decl and E.TARGET_ELLIP == 3 and E.Engine.TARGET_ELLIP == 3
    for other in (E.EXPORTED_SYMBOLS, E.DEBUG_SYMBOLS, E.SITE_SYMBOLS, E.SWD_ELLIP_SYMBOLS):
        assert not set(decl) & set(other)
    lib = C.CDLL(E.LIB_PATH)
    for name in decl:
        assert hasattr(lib, name), "missing export %s" % name
    # the drop-in header is as it was: no new kind, no new call, the same version
    base = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "bh_engine.h")).read(), flags=re.S)
    assert "ELLIP" not in base and "ellip" not in base
    assert lib.bh_abi_version() == 10
    for word in ("Failure.", "Values.", "Bits.", "never share a search with each other"):   # the contract of a fused call
        assert word in txt


# ---- the pure plan --------------------------------------------------------------------------------------------------------------
class PlanTarget(C.Structure):   # bh_ellip_plan_target
    _fields_ = [(k, C.c_int32) for k in ("kind", "iwave", "igr", "mode", "flsph", "n", "xid")]


def plan(targets, x_table=False):
    """targets: (kind, iwave, igr, mode, flsph, x) -> (source per target, searches added); the ids of the period arrays by their
    bits, as the engine assigns them at registration"""
    lib = C.CDLL(E.LIB_PATH)
    lib.bh_plan_ellip.restype = C.c_int
    lib.bh_plan_ellip.argtypes = [C.c_int, C.POINTER(PlanTarget), C.c_int, C.POINTER(C.c_int32)]
    ids = {}
    arr = (PlanTarget * 8)()
    for i, (kind, iwave, igr, mode, flsph, x) in enumerate(targets):
        xid = -1 if x is None else ids.setdefault(np.asarray(x, dtype=np.float64).tobytes(), len(ids))
        arr[i] = PlanTarget(kind, iwave, igr, mode, flsph, 0 if x is None else len(x), xid)
    src = (C.c_int32 * 8)(*([99] * 8))
    own = lib.bh_plan_ellip(len(targets), arr, int(x_table), src)
    return list(src)[:len(targets)], own


def swd(x=X, iwave=RAYLEIGH, igr=PHASE, mode=1, flsph=0):
    return (SWD, iwave, igr, mode, flsph, x)


ELL = (ELLIP, RAYLEIGH, PHASE, 1, 0, X)
RFT = (RF, 0, 0, 0, 0, None)
X_LAST_BIT = X.copy()
X_LAST_BIT[3] = np.nextafter(X[3], 100.0)
X61 = np.linspace(1.0, 40.0, 61)


@pytest.mark.parametrize("targets, x_table, want", [
    ([swd(), ELL], False, ([-2, 0], 0)),                       # shared with 0, no extra job
    ([ELL], False, ([-1], 1)),                                 # alone
    ([swd(iwave=LOVE), ELL], False, ([-2, -1], 1)),            # Love phase at the same periods
    ([swd(igr=GROUP), ELL], False, ([-2, -1], 1)),             # Rayleigh group
    ([swd(mode=2), ELL], False, ([-2, -1], 1)),                # Rayleigh phase, first overtone
    ([swd(x=X_LAST_BIT), ELL], False, ([-2, -1], 1)),          # one period differs in its last bit
    ([swd(), ELL], True, ([-2, -1], 1)),                       # a period table is in force
    ([swd(x=X61), (ELLIP, RAYLEIGH, PHASE, 1, 0, X61[:60])], False, ([-2, -1], 1)),   # the dispersion target runs on the 60-point grid
    ([RFT, swd(), ELL], False, ([-2, -2, 1], 0)),              # shared with 1
    ([swd(flsph=1), swd(), ELL], False, ([-2, -2, 1], 0)),     # the FIRST target that qualifies
    ([ELL, ELL], False, ([-1, -1], 2)),                        # two ellipticities: a search each
    ([swd(), ELL, ELL], False, ([-2, 0, 0], 0)),               # ... unless a dispersion target serves both
    ([swd(), (USER, 0, 0, 0, 0, None)], False, ([-2, -2], 0)),
])
def test_plan_shares_one_search_where_one_suffices(targets, x_table, want):
    assert plan(targets, x_table) == want


def test_plan_with_more_than_sixty_periods_compares_counts_not_only_ids():
    """a dispersion target of n > 60 periods never serves, even if an id were handed in equal"""
    lib = C.CDLL(E.LIB_PATH)
    lib.bh_plan_ellip.argtypes = [C.c_int, C.POINTER(PlanTarget), C.c_int, C.POINTER(C.c_int32)]
    arr = (PlanTarget * 2)(PlanTarget(SWD, RAYLEIGH, PHASE, 1, 0, 61, 0), PlanTarget(ELLIP, RAYLEIGH, PHASE, 1, 0, 61, 0))
    src = (C.c_int32 * 2)()
    assert lib.bh_plan_ellip(2, arr, 0, src) == 1 and list(src) == [-2, -1]
    assert lib.bh_plan_ellip(9, arr, 0, src) == -1 and lib.bh_plan_ellip(2, None, 0, src) == -1


def test_site_plan_counts_the_kind_as_a_forward_model():
    from test_site_plan import Ask, Target, library
    site_plan, text = library()
    for sites in (False, True):
        q = Ask(sites=sites, level=1 if sites else 0, nt=2)
        q.t[0], q.t[1] = Target(SWD, E.LAW_NOCORR), Target(ELLIP, E.LAW_NOCORR)
        p = site_plan(C.byref(q))
        assert (p.refusal, p.code) == (0, 0)
        q.t[1] = Target(USER, E.LAW_NOCORR)
        p = site_plan(C.byref(q))
        assert p.refusal == 1 and "BH_TARGET_USER" in text(p.refusal).decode()


# ---- the target -----------------------------------------------------------------------------------------------------------------
def ell_target(x=X, law="nocorr", fused=True, **params):
    t = bh.RayleighEllipticity(x, 0.8 + 0.0 * x, fused=fused)
    t.set_noise_law(law)
    if params:
        t.moddata.plugin.set_modelparams(**params)
    return t


def test_fused_target_is_engine_backed_and_describes_its_forward_model():
    t = ell_target()
    assert t.fused and t.engine_backed() and (t.ref, t.noiseref) == ("rellip", "ell")
    d = t.engine_desc()
    assert d["kind"] == E.TARGET_USER and d["n"] == X.size and d["law"] == E.LAW_NOCORR   # what bh_targets_set is told
    assert np.array_equal(d["x"], X) and d["x"].dtype == np.float64
    assert (d["nsteps"], d["signed"], d["ratio"]) == (2, False, "hv")
    t.moddata.plugin.set_modelparams(nsteps=0, signed=True, ratio="zh")
    d = t.engine_desc()
    assert (d["nsteps"], d["signed"], d["ratio"]) == (0, True, "zh")
    # the parameters are part of what a joint target registers: a change registers again
    jt = bh.JointTarget([t])
    s0 = jt._signature()
    t.moddata.plugin.set_modelparams(nsteps=1)
    assert jt._signature() != s0
    # a plugin of the user's own in its place: a user target again
    t.update_plugin(object())
    assert not t.engine_backed() and "nsteps" not in t.engine_desc()


def test_default_target_is_described_as_before():
    t0 = bh.RayleighEllipticity(X, 0.8 + 0.0 * X)
    t0.set_noise_law("nocorr")
    t1 = ell_target(fused=False)
    for t in (t0, t1):
        assert not t.fused and not t.engine_backed()
        d = t.engine_desc()
        assert sorted(d) == ["kind", "law", "n", "yobs"] and d["kind"] == E.TARGET_USER


def test_device_chains_still_refuse_the_default_target_only():
    """fused=False: the message as it was; the check itself lets a fused target through (what follows needs a GPU: tests/test_gpu_ellip_fused.py)"""
    from bayhunter_amd.Targets import RayleighEllipticity
    src = open(os.path.join(REPO, "bayhunter_amd", "device_chains.py")).read()
    assert "the ellipticity is not part of it yet (ChainBatch runs it)" in src
    with pytest.raises(E.EngineError, match="not part of it yet"):
        bh.DeviceChains([ell_target(fused=False)], nchains=4, initparams={"iter_burnin": 8, "iter_main": 8},
                        modelpriors={"ellnoise_corr": 0.0, "ellnoise_sigma": (0.01, 0.2)})
    assert isinstance(ell_target(), RayleighEllipticity)


# ---- the site set ---------------------------------------------------------------------------------------------------------------
def phase_target(x=X):
    t = bh.RayleighDispersionPhase(x, 3.0 + 0.02 * x)
    t.set_noise_law("nocorr")
    return t


def test_site_set_admits_the_fused_slot_and_names_what_it_refuses():
    SiteTargets([[phase_target(), ell_target()] for _ in range(3)]).check()
    SiteTargets([[phase_target(X[:n]), ell_target()] for n in (5, 4, 3)], per_site_x=True).check()
    SiteTargets([[phase_target(X[:n]), ell_target()] for n in (5, 4, 3)], per_site_x="all", per_site_corr=True).check()
    with pytest.raises(ValueError, match="a user plugin"):           # the default target: as before
        SiteTargets([[phase_target(), ell_target(fused=False)] for _ in range(2)]).check()
    with pytest.raises(ValueError, match=r"rellip.*missing=True.*RayleighEllipticity"):
        SiteTargets([[phase_target(), ell_target()], [phase_target(), ell_target()]], per_site_x="all", missing=True).check()
    with pytest.raises(ValueError, match=r"rellip.*missing=True.*RayleighEllipticity"):
        SiteTargets([[phase_target(), ell_target()], [phase_target(), None]], per_site_x="all", missing=True).check()
    other = X.copy()
    other[2] = 9.0
    for flag in (False, True, "all"):                                # periods per site are the dispersion slots', not this one's
        with pytest.raises(ValueError, match=r"rellip.*x differs"):
            SiteTargets([[phase_target(), ell_target()], [phase_target(), ell_target(other)]], per_site_x=flag).check()
    with pytest.raises(ValueError, match=r"rellip.*ellipticity parameters \(nsteps, signed, ratio\) \(1, False, 'hv'\)"):
        SiteTargets([[phase_target(), ell_target()], [phase_target(), ell_target(nsteps=1)]]).check()
    with pytest.raises(ValueError, match=r"rellip.*ellipticity parameters"):
        SiteTargets([[phase_target(), ell_target()], [phase_target(), ell_target(ratio="zh")]]).check()
