"""Sites that lack some of the array's targets (include/bh_engine_sites_missing.h, SiteTargets(missing=True)), the parts that need
no GPU: the header and the library's exports, what SiteTargets accepts and refuses with and without `missing`, the tables it
registers (count 0 and placeholders), the slot layout of noise and misfits and its way back, `site(s)`, and -- with the oracle --
that the batches of tests/test_gpu_sites_missing.py are not about failed rows."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, golden
import bayhunter_amd as bh
from bayhunter_amd.sites import SiteTargets, ABSENT_NOISE, gather_slots, scatter_slots, slot_columns
from test_sites_x_host import X_FULL, X_SETS, _RecordingEngine


def test_library_exports_the_missing_header():
    from bayhunter_amd import engine as E
    txt = open(os.path.join(REPO, "include", "bh_engine_sites_missing.h")).read()
    assert '#include "bh_engine_sites_x_all.h"' in txt
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decl = sorted(set(re.findall(r"\b(bh_[a-z_]+)\s*\(", txt)))
    assert decl == ["bh_chain_propose_sites", "bh_chain_propose_window_sites", "bh_sites_set_missing"]
    assert sorted(E.SITE_MISSING_SYMBOLS) == decl
    for other in (E.EXPORTED_SYMBOLS, E.DEBUG_SYMBOLS, E.SITE_SYMBOLS, E.SITE_RF_SYMBOLS, E.SITE_X_SYMBOLS, E.SITE_X_ALL_SYMBOLS,
                  E.POSTERIOR_SYMBOLS):
        assert not set(decl) & set(other)
    lib = ctypes.CDLL(E.LIB_PATH)
    for name in decl:
        assert hasattr(lib, name), "missing export %s" % name
    for hdr in ("bh_engine.h", "bh_engine_debug.h", "bh_engine_sites.h", "bh_engine_sites_rf.h", "bh_engine_sites_x.h",
                "bh_engine_sites_x_all.h", "bh_engine_posterior.h"):   # declared in the new header only
        other = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", hdr)).read(), flags=re.S)
        assert not any(re.search(r"\b%s\b" % name, other) for name in decl), hdr
    lib.bh_abi_version.restype = ctypes.c_int
    assert lib.bh_abi_version() == 10                            # extension headers are outside the contract


def slots_of(g, x, dy=0.0, have="111", law_l="nocorr", p=6.4, love_cls=None):
    """[Rayleigh phase, Love phase, P receiver function] of a site at periods x, None where `have` says 0"""
    x = np.asarray(x, dtype=float)
    t1 = bh.RayleighDispersionPhase(x, 3.4 + 0.01 * x + dy)
    t1.set_noise_law("nocorr")
    t2 = (love_cls or bh.LoveDispersionPhase)(x[::2], 3.7 + 0.012 * x[::2] + dy, yerr=0.01 + 0.001 * np.arange(x[::2].size))
    t2.set_noise_law(law_l)
    t3 = bh.PReceiverFunction(g["xrf"], g["yrf"] * (1.0 + dy))
    t3.moddata.plugin.set_modelparams(gauss=1.0, p=p)
    t3.set_noise_law("exp")
    return [t if c == "1" else None for t, c in zip((t1, t2, t3), have)]


HAVE = ["111", "101", "011", "110"]


def four_sites(g, **kw):
    return [slots_of(g, X_SETS[s], 0.01 * s, HAVE[s], **kw) for s in range(4)]


def test_missing_accepts_none_slots_and_describes_the_slots():
    g = golden("chain_golden.npz")
    rows = four_sites(g)
    st = SiteTargets(rows, per_site_x="all", missing=True)
    st.check()
    assert st.missing and st.nsites == 4 and st.ntargets == 3
    assert np.array_equal(st.present, [[c == "1" for c in h] for h in HAVE])
    # the slots' descriptors: the first site that has each
    assert st.targets[0] is rows[0][0] and st.targets[1] is rows[0][1] and st.targets[2] is rows[0][2]
    st2 = SiteTargets(rows[1:], per_site_x="all", missing=True)
    assert st2.targets[0] is rows[1][0] and st2.targets[1] is rows[2][1] and st2.targets[2] is rows[1][2]
    # site(s): exactly the targets the site has, in order -- the one-site run
    for s, row in enumerate(rows):
        jt = st.site(s)
        assert isinstance(jt, bh.JointTarget) and jt.ntargets == HAVE[s].count("1")
        assert all(a is b for a, b in zip(jt.targets, [t for t in row if t is not None]))
    # sites given as JointTargets have every slot
    full = SiteTargets([bh.JointTarget(slots_of(g, X_FULL)), slots_of(g, X_SETS[1], have="100")], per_site_x="all", missing=True)
    full.check()
    assert np.array_equal(full.present, [[True, True, True], [True, False, False]])
    assert not SiteTargets([bh.JointTarget(slots_of(g, X_FULL))]).missing


def test_missing_refusals():
    g = golden("chain_golden.npz")
    M = dict(per_site_x="all", missing=True)
    with pytest.raises(ValueError, match="site 1 has no target"):
        SiteTargets([slots_of(g, X_FULL), slots_of(g, X_FULL, have="000")], **M)
    with pytest.raises(ValueError, match="slot 1 is present at no site"):
        SiteTargets([slots_of(g, X_FULL, have="101"), slots_of(g, X_FULL, have="100")], **M)
    with pytest.raises(ValueError, match="site 1 gives 2 slots, site 0 gives 3"):
        SiteTargets([slots_of(g, X_FULL), slots_of(g, X_FULL)[:2]], **M)
    for psx in (False, True):
        with pytest.raises(ValueError, match="missing=True needs per_site_x=\"all\""):
            SiteTargets(four_sites(g), per_site_x=psx, missing=True)
    # a class mismatch within a slot, among the sites that have it (site 0 lacks it)
    rows = [slots_of(g, X_FULL, have="101"), slots_of(g, X_SETS[1]), slots_of(g, X_SETS[2], love_cls=bh.LoveDispersionGroup)]
    with pytest.raises(ValueError, match=r"site 2 \(site002\), slot 1 \(ldispgr\) is a LoveDispersionGroup, site 1's is a LoveDispersionPhase"):
        SiteTargets(rows, **M).check()
    # ... a law mismatch, a receiver-function parameter mismatch without per_site_rf
    with pytest.raises(ValueError, match="noise law 'exp', site 0's 'nocorr'"):
        SiteTargets([slots_of(g, X_FULL), slots_of(g, X_SETS[1], law_l="exp"), slots_of(g, X_FULL, have="100")], **M).check()
    with pytest.raises(ValueError, match="receiver-function parameters"):
        SiteTargets([slots_of(g, X_FULL), slots_of(g, X_SETS[1], p=7.0), slots_of(g, X_FULL, have="110")], **M).check()
    SiteTargets([slots_of(g, X_FULL), slots_of(g, X_SETS[1], p=7.0), slots_of(g, X_FULL, have="110")], per_site_rf=True, **M).check()
    # the Gauss law on a slot that some site lacks; present everywhere it is served as before
    def gauss_rf(have):
        row = slots_of(g, X_FULL, have=have)
        if row[2] is not None:
            row[2].set_noise_law("gauss", corr=0.5, rcond=1e-5)
        return row
    with pytest.raises(ValueError, match="Gauss law on a slot that some site lacks"):
        SiteTargets([gauss_rf("111"), gauss_rf("110")], **M).check()
    SiteTargets([gauss_rf("111"), gauss_rf("011")], **M).check()


def test_without_missing_none_slots_and_differing_target_lists_are_refused_as_before():
    g = golden("chain_golden.npz")
    rows = four_sites(g)
    with pytest.raises((ValueError, AttributeError, TypeError)):          # a None slot is no target
        SiteTargets(rows, per_site_x="all").check()
    lists = [[t for t in row if t is not None] for row in rows]
    with pytest.raises(ValueError, match="site 1 \\(site001\\) has 2 targets, site 0 has 3"):
        SiteTargets(lists, per_site_x="all").check()
    with pytest.raises(ValueError, match="is a PReceiverFunction, site 0's is a LoveDispersionPhase"):
        SiteTargets([lists[1] + [lists[1][1]], lists[0]][::-1], per_site_x="all", per_site_rf=True).check()


class _RecordingEngineMissing(_RecordingEngine):
    def set_sites_missing(self, n, x, yobs, yerr=None):
        self.calls.append(("sites_missing", n.copy(), x.copy(), yobs.copy(), None if yerr is None else yerr.copy()))

    def set_sites_x_all(self, n, x, yobs, yerr=None):
        self.calls.append(("sites_x_all", n.copy(), x.copy(), yobs.copy(), None if yerr is None else yerr.copy()))


def test_registration_holds_count_zero_and_placeholders_and_always_the_rf_table():
    g = golden("chain_golden.npz")
    nrf = np.size(g["xrf"])
    rows = [slots_of(g, X_SETS[s], 0.01 * s, HAVE[s], law_l="nocorr_scalederr", p=5.5 + s) for s in range(4)]
    eng = _RecordingEngineMissing()
    st = SiteTargets(rows, engine=eng, per_site_x="all", per_site_rf=True, missing=True)
    st._register()
    st._register()
    assert [c[0] for c in eng.calls] == ["targets", "sites_missing", "sites_rf"]
    descs = eng.calls[0][1]
    kl = [X_SETS[s][::2].size for s in range(4)]
    assert [d["n"] for d in descs] == [30, 15, nrf]             # capacities: the largest count among the sites that have the slot
    for d in descs[:2]:
        assert np.all(d["x"] == 1.0) and np.all(d["yobs"] == 0.0) and np.size(d["x"]) == d["n"]
    assert np.all(descs[1]["yerr"] == 1.0) and descs[2]["p"] == 5.5
    _, n, x, yobs, yerr = eng.calls[1]
    assert n.dtype == np.int32
    assert np.array_equal(n, [[30, kl[0], nrf], [15, 0, nrf], [0, kl[2], nrf], [1, kl[3], 0]])
    off = [0, 30, 45, 45 + nrf]
    assert x.shape == yobs.shape == yerr.shape == (4, off[-1])
    for s, row in enumerate(rows):
        for t, tg in enumerate(row):
            lo, hi = off[t], off[t + 1]
            if tg is None:                                      # placeholders: x 0, yobs 0, yerr 1
                assert np.all(x[s, lo:hi] == 0.0) and np.all(yobs[s, lo:hi] == 0.0) and np.all(yerr[s, lo:hi] == 1.0)
                continue
            k = n[s, t]
            assert np.array_equal(x[s, lo:lo + k], tg.obsdata.x) and np.all(x[s, lo + k:hi] == 0.0)
            assert np.array_equal(yobs[s, lo:lo + k], tg.obsdata.y) and np.all(yobs[s, lo + k:hi] == 0.0)
    assert np.array_equal(yerr[0, 30:30 + kl[0]], rows[0][1].obsdata.yerr)
    _, p, nsv = eng.calls[2]                                    # p / nsv from every site's own plugin, 0 where it has none
    assert np.array_equal(p[:, 2], [5.5, 6.5, 7.5, 0.0]) and np.all(p[:, :2] == 0.0) and np.all(nsv == 0.0)
    # the table of receiver-function parameters is registered whether or not per_site_rf is set
    eng2 = _RecordingEngineMissing()
    SiteTargets(four_sites(g), engine=eng2, per_site_x="all", missing=True)._register()
    assert [c[0] for c in eng2.calls] == ["targets", "sites_missing", "sites_rf"]
    assert np.array_equal(eng2.calls[2][1][:, 2], [6.4, 6.4, 6.4, 0.0])
    # without missing: the entry point of per_site_x="all", as before
    eng3 = _RecordingEngineMissing()
    SiteTargets([slots_of(g, X_SETS[s]) for s in range(3)], engine=eng3, per_site_x="all")._register()
    assert [c[0] for c in eng3.calls] == ["targets", "sites_x_all"]


def test_engine_method_passes_the_arrays_to_the_new_entry_points():
    from bayhunter_amd import engine as E

    class Lib(object):
        def __init__(self):
            self.calls = []

        def bh_sites_set_missing(self, *a):
            self.calls.append(("missing", a[1]))
            return 0

        def bh_chain_propose_window(self, *a):
            self.calls.append(("propose", len(a)))
            return 0

        def bh_chain_propose_window_sites(self, *a):
            self.calls.append(("propose_sites", a[-1]))
            return 0

        def bh_engine_stream(self, h):
            return None

    eng = E.Engine.__new__(E.Engine)
    eng._L, eng._h, eng.ldy, eng.ntargets = Lib(), None, 5, 2
    n = np.array([[2, 3], [0, 2], [2, 0]], np.int32)
    eng.set_sites_missing(n, np.ones((3, 5)), np.zeros((3, 5)))
    assert eng._L.calls == [("missing", 3)] and eng.nsites == 3
    with pytest.raises(ValueError, match="n must have shape"):
        eng.set_sites_missing(n[:2], np.ones((3, 5)), np.zeros((3, 5)))
    cfg, st = E.ChainConfig(), E.ChainState()
    eng.chain_propose_window(cfg, st, 4, 0, 1, 4)
    eng.chain_propose_window(cfg, st, 4, 0, 1, 4, absent=1234)
    assert eng._L.calls[1:] == [("propose", 7), ("propose_sites", 1234)]


def test_slot_layout_round_trips():
    present = np.array([True, False, True, True, False])
    ncol, mcol = slot_columns(present)
    assert np.array_equal(ncol, [0, 1, 4, 5, 6, 7]) and np.array_equal(mcol, [0, 2, 3, 5])
    rs = np.random.RandomState(0)
    for lead in ((), (7,), (3, 4)):
        noise, mis = rs.uniform(0.1, 1, lead + (6,)), rs.uniform(0.1, 1, lead + (4,))
        sn, sm = scatter_slots(present, noise, mis)
        assert sn.shape == lead + (10,) and sm.shape == lead + (6,)
        assert np.all(sn[..., [2, 3, 8, 9]] == ABSENT_NOISE) and np.all(sm[..., [1, 4]] == 0.0)
        assert np.array_equal(sm[..., 5], mis[..., 3])         # the joint misfit stays last
        gn, gm = gather_slots(present, sn, sm)
        assert np.array_equal(gn, noise) and np.array_equal(gm, mis)
    everything = np.ones(3, bool)
    sn, sm = scatter_slots(everything, np.arange(6.0), np.arange(4.0))
    assert np.array_equal(sn, np.arange(6.0)) and np.array_equal(sm, np.arange(4.0))


def test_the_gpu_tests_batches_are_not_about_failed_rows(oracle):
    """tests/test_gpu_sites_missing.py compares whole rows, failed models included.  With the oracle alone: for every batch it
    uses, every site has models, every (slot, present) and (slot, absent) combination has models, and of the models of every
    (site, present dispersion slot) fewer than half fail -- while failed rows do take part in every batch.  (A receiver function
    does not fail in the oracle.)  Fixed seeds: fixed shares."""
    import test_gpu_sites_missing as T
    from test_gpu_sites_x import NSITES
    uses = [("full", name) for name, _ in T.REF_BATCHES] + [("phase_rf", b) for b in ("synth8", "prior21", "small21")] + \
           [("group_mix", b) for b in ("prior21", "small21")]
    seen = {}
    for structure, which in uses:
        slots = T.STRUCTURES[structure][0]
        present = T.present_of(structure)
        assert present.any(axis=1).all() and present.any(axis=0).all() and (~present).any(axis=0).all()
        nlay, h, vp, vs, rho, site = dict(T.REF_BATCHES)[which]()
        counts = np.bincount(site, minlength=NSITES)
        assert counts.min() >= 8, (which, counts)
        for t in range(len(slots)):                              # models with the slot and models without it
            assert counts[present[:, t]].sum() > 0 and counts[~present[:, t]].sum() > 0
        failed_any = False
        for s in range(NSITES):
            m = site == s
            for t, spec in enumerate(slots):
                if not present[s, t] or spec[0] != "swd":
                    continue
                per = T.slot_periods(spec, s)
                key = (which, s, spec[1], spec[2], spec[3], per.tobytes())
                if key not in seen:
                    _, e, _ = oracle.swd_batch(nlay[m], h.T[m], vp.T[m], vs.T[m], rho.T[m], per, spec[1], spec[2], mode=spec[3])
                    seen[key] = float((e != 0).mean())
                assert seen[key] < 0.5, (structure, which, s, t, seen[key])
                failed_any = failed_any or seen[key] > 0.0
        assert failed_any, (structure, which)
