"""Sites with their own noise law on the MI355X (include/bh_engine_sites_laws.h, SiteTargets(per_site_law=True)).
The rule under test: a model of site s gets, on every target, what a call over the same batch gives it in which EVERY site has site
s's laws -- bit for bit.  The reference of (a) is therefore the project's own existing path (the count table without a law table,
the law in the descriptor), evaluated once per distinct row of the law table over the WHOLE batch (same B, same capacities: same
launch forms and slabs); no tolerance.  (b) holds everything to tests/like_ref.py within that module's own a priori bound times
its FACTOR.

The receiver-function kernels set no failure flag, so "a failure flag on a slot the site lacks" needs a site that lacks the
DISPERSION slot: the layout "swd_lacked" takes site 3's curve away (the layout "rf_lacked" is the one every other case uses: site 5
has no receiver function)."""
import os

import numpy as np
import pytest

from conftest import golden
import bayhunter_amd as bh
import like_ref as LR
from bayhunter_amd import engine as E
from bayhunter_amd.device_chains import DeviceChains
from bayhunter_amd.synth import synth_models
from bayhunter_amd.Targets import LAWS as LAW_CODES
from test_gpu_like_paths import tuned
from test_gpu_sites import eval_device
from test_gpu_sites_gauss import gauss_class, same_samples
from test_gpu_sites_x import PRIORS, bits

pytestmark = pytest.mark.gpu

NOCORR, SCALED, EXP, GAUSS = E.LAW_NOCORR, E.LAW_NOCORR_SCALED, E.LAW_EXP, E.LAW_GAUSS
NSITES, CAP = 6, 30
CNT0 = (30, 17, 1, 2, 9, 24)                        # periods of every site: an exp site with ONE sample (the n == 1 edge term), one with two
LAW0 = (NOCORR, SCALED, EXP, EXP, NOCORR, SCALED)   # the dispersion slot
LAW1 = (GAUSS, GAUSS, EXP, NOCORR, SCALED, None)    # the receiver function; site 5 lacks it
CLASS_MIX = np.array([0, 1, -1, -1, -1, -1], dtype=np.int32)
CORRS, OTHER_CORRS = (0.90, 0.96), (0.94, 0.98)
# (n of the receiver function, B, rows per site): n = 30 -> one wavefront per model, n = 200 -> one workgroup per model
CASES = {"n30": (30, 132, (30, 25, 20, 20, 20, 15)), "n200": (200, 300, (70, 60, 50, 45, 40, 33))}


class Setup(object):
    """6 sites over [Rayleigh phase, P receiver function of n samples].  EVERY site carries finite errors on both slots and a
    matrix, so any law can be installed anywhere (the comparison evaluations install one site's laws at all of them)."""

    def __init__(self, n, seed, lack_swd=None):
        rs = np.random.RandomState(seed)
        self.n, self.ldy = n, CAP + n
        self.cnt = np.array([[CNT0[s], n if LAW1[s] is not None else 0] for s in range(NSITES)], dtype=np.int32)
        if lack_swd is not None:
            self.cnt[lack_swd, 0] = 0
        self.law = np.array([[LAW0[s], GAUSS if LAW1[s] is None else LAW1[s]] for s in range(NSITES)], dtype=np.int32)
        self.x, self.yobs, self.yerr = np.zeros((NSITES, self.ldy)), np.zeros((NSITES, self.ldy)), np.ones((NSITES, self.ldy))
        for s in range(NSITES):
            k = self.cnt[s, 0]
            per = np.linspace(2.0 + s, 60.0 - 2 * s, CNT0[s])[:k]
            self.x[s, :k] = per
            self.yobs[s, :k] = 3.0 + 0.02 * per + rs.normal(0, 0.05, k)
            self.yerr[s, :k] = rs.uniform(0.02, 0.06, k)
            if self.cnt[s, 1]:
                self.yobs[s, CAP:] = rs.normal(0, 0.05, n)
                self.yerr[s, CAP:] = rs.uniform(0.02, 0.06, n)
        self.p = np.zeros((NSITES, 2))
        self.p[self.cnt[:, 1] > 0, 1] = 6.4
        self.nsv = np.zeros((NSITES, 2))

    def classes(self, corrs=CORRS):
        mats = [gauss_class(self.n, c) for c in corrs]
        return np.stack([m[0] for m in mats]), np.array([m[1] for m in mats])

    def descs(self, l0, l1, corr=CORRS[0]):
        """the capacity descriptors with laws (l0, l1): placeholders for the data, the site path reads the tables"""
        d0 = dict(kind=E.TARGET_SWD, law=l0, n=CAP, x=np.ones(CAP), yobs=np.zeros(CAP), iwave=2, igr=0)
        d1 = dict(kind=E.TARGET_RF, law=l1, n=self.n, waveno=0, p=6.4, gauss=2.5, tshift=5.0, nsamp=512, fsamp=5.0, yobs=np.zeros(self.n))
        for d in (d0, d1):
            if d["law"] == SCALED:
                d["yerr"] = np.ones(d["n"])
        if l1 == GAUSS:
            d1["rinv"], d1["logdet_r"] = gauss_class(self.n, corr)
        return [d0, d1]

    def register_mixed(self, eng, corrs=CORRS, upto="gauss"):
        eng.set_targets(self.descs(NOCORR, GAUSS))
        eng.set_sites_missing_gauss(self.cnt, self.x, self.yobs, self.yerr)
        eng.set_sites_rf(self.p, self.nsv)
        if upto == "rf":
            return
        eng.set_sites_laws(self.law, self.yerr)
        if upto == "gauss":
            eng.set_sites_gauss(1, CLASS_MIX, *self.classes(corrs))

    def register_parent(self, eng, l0, l1, c):
        """the existing path: no law table, laws (l0, l1) in the descriptors, hence at every site; Gauss: every site that has the
        receiver function in class c"""
        eng.set_targets(self.descs(l0, l1))
        eng.set_sites_missing_gauss(self.cnt, self.x, self.yobs, self.yerr)
        eng.set_sites_rf(self.p, self.nsv)
        if l1 == GAUSS:
            eng.set_sites_gauss(1, np.where(self.cnt[:, 1] > 0, c, -1).astype(np.int32), *self.classes())

    def law_rows(self):
        """the distinct rows of the law table as (l0, l1, class, sites that have that row); a lacked slot's law is not read: the
        comparison installs EXP there"""
        out = {}
        for s in range(NSITES):
            key = (LAW0[s], EXP if LAW1[s] is None else LAW1[s], int(max(CLASS_MIX[s], 0)))
            out.setdefault(key, []).append(s)
        return [k + (v,) for k, v in sorted(out.items())]

    def site_ref_descs(self, s, corrs=CORRS):
        """site s's own descriptors over its own samples, for like_ref.joint_ref, and the columns of ymod / noise they take"""
        ds, ycol, ncol = [], [], []
        for t, (lo, law) in enumerate(((0, LAW0[s]), (CAP, LAW1[s]))):
            k = int(self.cnt[s, t])
            if k == 0:
                continue
            d = dict(law=law, n=k, yobs=self.yobs[s, lo:lo + k], yerr=self.yerr[s, lo:lo + k])
            if law == GAUSS:
                d["rinv"], d["logdet_r"] = gauss_class(self.n, corrs[CLASS_MIX[s]])
            ds.append(d)
            ycol += list(range(lo, lo + k))
            ncol += [2 * t, 2 * t + 1]
        return ds, np.array(ycol), np.array(ncol)


def site_rows(counts, bad_at):
    """the site of every row: the sites' rows interleaved round robin, two rows (at bad_at) out of range"""
    left, order = list(counts), []
    while any(left):
        for s in range(NSITES):
            if left[s]:
                order.append(s)
                left[s] -= 1
    for pos, val in zip(bad_at, (-1, NSITES)):
        order.insert(pos, val)
    return np.array(order, dtype=np.int32)


def batch(rs, B):
    """B models; every 13th from the 3rd has an absurd top layer: its dispersion fails (a receiver function never sets the flag)"""
    nlay, h, vp, vs, rho = synth_models(rs, B, 10, ragged=True)
    absurd = np.zeros(B, bool)
    absurd[3::13] = True
    vs[0, absurd] = 200.0
    noise = np.column_stack([rs.uniform(0.1, 0.6, B) if i % 2 == 0 else rs.uniform(0.02, 0.1, B) for i in range(4)])
    return (nlay, h, vp, vs, rho), noise, absurd


def run_case(eng, case, tile, lack_swd=None):
    n, B, counts = CASES[case]
    S = Setup(n, 2000 + n, lack_swd)
    rs = np.random.RandomState(77 + n)
    models, noise, absurd = batch(rs, B)
    site = site_rows(counts, (7, B - 5))
    assert site.size == B
    inrange = (site >= 0) & (site < NSITES)
    has0 = np.zeros(B, bool)
    has0[inrange] = S.cnt[site[inrange], 0] > 0
    want_err = ~inrange | (absurd & has0)                  # the rows failed on purpose: out of range, or absurd on a slot the site HAS
    # absurd on a slot the site LACKS: not failed -- the flag is not read -- but the receiver function of such a model is no number,
    # so (a) holds them to the comparison's bits and (b) leaves exactly them out beside the failed ones
    unread = absurd & inrange & ~has0
    what = "%s tile %d" % (case, tile)
    with tuned(eng, "gauss_tile", tile):
        S.register_mixed(eng)
        got = eval_device(eng, models, noise, site, S.ldy)
        again = eval_device(eng, models, noise, site, S.ldy)
        for a, b in zip(got, again):
            assert np.array_equal(bits(a), bits(b)), what + ": not repeatable"
        print("%s: %d rows, %d failed, %d wanted (absurd %d, of them on a lacked slot %d)"
              % (what, B, int((got[2] != 0).sum()), int(want_err.sum()), int(absurd.sum()), int((absurd & inrange & ~has0).sum())))
        assert np.array_equal(got[2] != 0, want_err), what + ": the failed rows are not exactly the deliberate ones"
        assert (absurd & has0).sum() >= 3 and (unread.sum() >= 3 if lack_swd is not None else unread.sum() == 0)
        for k in np.flatnonzero(~inrange):                 # a site out of range fails in band
            assert got[2][k] == 1 and got[0][k] == -1e15 and np.all(got[1][k] == 1e15)
        # (a) one comparison evaluation per distinct row of the law table, through the path without a law table
        for l0, l1, c, sites in S.law_rows():
            S.register_parent(eng, l0, l1, c)
            ref = eval_device(eng, models, noise, site, S.ldy)
            m = np.isin(site, sites)
            assert m.any()
            for k, name in enumerate(("logL", "misfits", "err", "ymod")):
                assert np.array_equal(bits(got[k][m]), bits(ref[k][m])), "%s: %s of the sites %r under laws (%d, %d)" % (what, name, sites, l0, l1)
    # (b) everything against the extended-precision reference, site by site over the site's own samples
    compared = 0
    for s in range(NSITES):
        m = np.flatnonzero((site == s) & (got[2] == 0) & ~unread)
        ds, ycol, ncol = S.site_ref_descs(s)
        ref, misf, bound, mb = LR.joint_ref(ds, got[3][m][:, ycol], noise[m][:, ncol])
        assert np.all(np.isfinite(bound)) and np.all(np.isfinite(ref.astype(float))), "%s site %d: a non-finite reference or bound" % (what, s)
        print("%s site %d: %d rows, max |logL - ref| / bound %.3g" % (what, s, m.size, float(np.max(np.abs(got[0][m] - ref).astype(float) / bound))))
        LR.assert_within(got[0][m], ref, bound, "%s site %d logL" % (what, s))
        present = np.flatnonzero(S.cnt[s] > 0)
        LR.assert_within(got[1][m][:, list(present) + [2]], misf, mb, "%s site %d misfits" % (what, s))
        assert np.all(got[1][m][:, np.flatnonzero(S.cnt[s] == 0)] == 0.0)
        compared += m.size
    assert compared == B - int(want_err.sum()) - int(unread.sum())   # left out: exactly the rows made absurd or put out of range on purpose
    assert np.all(got[2][unread] == 0) and np.all(got[1][unread, 0] == 0.0)
    return S, models, noise, site, got


@pytest.mark.parametrize("case,tile", [("n30", 64), ("n30", 128), ("n200", 64), ("n200", 128)])
def test_every_model_gets_its_own_sites_law(engine, case, tile):
    run_case(engine, case, tile)


@pytest.mark.parametrize("case", ["n30", "n200"])
def test_a_failure_flag_on_a_slot_the_site_lacks_is_not_read(engine, case):
    run_case(engine, case, 0, lack_swd=3)


@pytest.mark.parametrize("case,lack_swd", [("n30", None), ("n200", None), ("n200", 3)])
def test_in_kernel_matvec_with_a_law_table(engine, case, lack_swd):
    """no_mfma (read when an engine is created): a site under another law reads no matrix"""
    before = engine.tuning("no_mfma")
    engine.set_tuning("no_mfma", 1)
    eng = None
    try:
        eng = E.Engine(0)
        eng.set_swd_search("reference")
        eng.set_swd_arith("exact")
        run_case(eng, case, 0, lack_swd)
    finally:
        if eng is not None:
            eng.close()
        engine.set_tuning("no_mfma", before)


def test_the_rows_of_a_site_under_another_law_enter_no_tile(engine):
    n, B, counts = CASES["n200"]
    S = Setup(n, 2000 + n)
    models, noise, _ = batch(np.random.RandomState(5), B)
    site = site_rows(counts, (7, B - 5))
    site[[7, B - 5]] = 5                                   # (the host entry refuses a site out of range)
    nlay, h, vp, vs, rho = models
    S.register_mixed(engine)
    before = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho)
    engine.set_sites_gauss(1, CLASS_MIX, *S.classes(OTHER_CORRS))
    after = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho)
    gauss_rows = np.isin(site, [0, 1])
    ok = before[2] == 0
    assert np.array_equal(before[2], after[2]) and (ok & gauss_rows).any() and (ok & ~gauss_rows).any()
    for k in range(2):                                     # logL and the misfits of the other sites: the same bits
        assert np.array_equal(bits(before[k][~gauss_rows]), bits(after[k][~gauss_rows]))
    assert np.all(before[0][ok & gauss_rows] != after[0][ok & gauss_rows])
    # ... and they lie within like_ref's bound of the OTHER matrices, site by site
    got = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
    for s in (0, 1):
        m = np.flatnonzero((site == s) & ok)
        ds, ycol, ncol = S.site_ref_descs(s, OTHER_CORRS)
        ref, _, bound, _ = LR.joint_ref(ds, got[3][m][:, ycol], noise[m][:, ncol])
        LR.assert_within(got[0][m], ref, bound, "other matrices, site %d" % s)


def test_entry_point_refusals_and_the_tables_lifetime(engine):
    n, B, counts = CASES["n30"]
    S = Setup(n, 2000 + n)
    models, noise, _ = batch(np.random.RandomState(9), B)
    nlay, h, vp, vs, rho = models
    site = site_rows(counts, (7, B - 5))
    site[[7, B - 5]] = 5
    L, hd = engine._L, engine._h
    P = lambda a: None if a is None else a.ctypes.data
    ev = lambda: engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho)

    def rc(law=S.law, yerr=S.yerr, nsites=NSITES):
        law = None if law is None else np.ascontiguousarray(law, dtype=np.int32)
        return L.bh_sites_set_laws(hd, nsites, P(law), P(yerr))

    def last():
        return L.bh_engine_last_error(hd)

    engine.set_targets(S.descs(NOCORR, GAUSS))
    flat = engine.evaluate_batch(nlay, h, vp, vs, noise, rho=rho)         # (for the last check: bh_evaluate_batch never reads the table)
    assert rc() == E.BH_EINVAL and b"no site table" in last()
    engine.set_sites(S.yobs)
    assert rc() == E.BH_EINVAL and b"no count table" in last()            # bh_sites_set registers no counts
    engine.set_sites_missing_gauss(S.cnt, S.x, S.yobs, S.yerr)
    engine.set_sites_rf(S.p, S.nsv)
    assert rc() == E.BH_OK
    assert rc(nsites=NSITES - 1) == E.BH_EINVAL and b"nsites" in last()
    assert rc(law=None) == E.BH_EINVAL
    bad = S.law.copy()
    bad[2, 0] = GAUSS                                                      # law 3 on a descriptor that is not under it
    assert rc(law=bad) == E.BH_EINVAL and b"BH_LAW_GAUSS" in last()
    for unknown in (4, -1):
        bad = S.law.copy()
        bad[3, 1] = unknown
        assert rc(law=bad) == E.BH_EINVAL and b"unknown" in last()
    ok = S.law.copy()
    ok[5, 1] = 77                                                          # where the count is 0 the entry is not read
    assert rc(law=ok) == E.BH_OK
    assert rc(yerr=None) == E.BH_EINVAL and b"yerr" in last()              # the table has pairs under law 1
    for val in (0.0, -0.01, np.nan, np.inf):
        ye = S.yerr.copy()
        ye[1, 5] = val                                                     # site 1's curve: law 1, 17 samples
        assert rc(yerr=ye) == E.BH_EINVAL and b"finite and positive" in last()
        ye = S.yerr.copy()
        ye[1, 20] = val                                                    # ... beyond its count: not read
        ye[0, 3] = val                                                     # ... and inside the count of a site under another law: not read
        assert rc(yerr=ye) == E.BH_OK
    # the class table under a law table: a class exactly for the sites under the Gauss law
    assert rc() == E.BH_OK
    with pytest.raises(E.EngineError, match="bh_sites_set_gauss"):         # a Gauss-law descriptor with sites under another law needs it
        ev()
    for wrong in ([0, 1, 0, -1, -1, -1], [0, -1, -1, -1, -1, -1], [0, 1, -1, -1, -1, 0]):
        with pytest.raises(E.EngineError, match="bh_sites_set_gauss"):
            engine.set_sites_gauss(1, wrong, *S.classes())
    engine.set_sites_gauss(1, CLASS_MIX, *S.classes())
    mixed = ev()
    assert (mixed[2] == 0).any()
    assert rc() == E.BH_OK                                                 # the law table drops the class tables
    with pytest.raises(E.EngineError, match="bh_sites_set_gauss"):
        ev()
    engine.set_sites_gauss(1, CLASS_MIX, *S.classes())
    assert np.array_equal(bits(ev()[0]), bits(mixed[0]))
    # the count table of bh_sites_set_axes takes the law table as well: the same bits
    engine.set_targets(S.descs(NOCORR, GAUSS))
    engine.set_sites_axes(S.cnt, S.x, S.yobs, S.yerr)
    engine.set_sites_rf(S.p, S.nsv)
    engine.set_sites_laws(S.law, S.yerr)
    engine.set_sites_gauss(1, CLASS_MIX, *S.classes())
    for a, b in zip(ev(), mixed):
        assert np.array_equal(bits(a), bits(b))
    # a count table drops the laws: the next evaluate behaves as without them -- the descriptors' laws at every site
    parent_cls = np.where(S.cnt[:, 1] > 0, CLASS_MIX.clip(0), -1).astype(np.int32)
    S.register_parent(engine, NOCORR, GAUSS, 0)
    engine.set_sites_gauss(1, parent_cls, *S.classes())
    parent = ev()
    S.register_mixed(engine)
    engine.set_sites_missing_gauss(S.cnt, S.x, S.yobs, S.yerr)
    engine.set_sites_rf(S.p, S.nsv)
    with pytest.raises(E.EngineError, match="has the target"):             # (no law table: -1 only where the count is 0)
        engine.set_sites_gauss(1, CLASS_MIX, *S.classes())
    engine.set_sites_gauss(1, parent_cls, *S.classes())
    dropped = ev()
    for a, b in zip(dropped, parent):
        assert np.array_equal(bits(a), bits(b))
    differ = np.isin(site, [1, 2, 3, 4]) & (mixed[2] == 0)                 # the sites whose laws are not the descriptors'
    assert np.all(dropped[0][differ] != mixed[0][differ])
    S.register_mixed(engine)
    engine.set_sites_rf(S.p, S.nsv)                                        # ... and so does a receiver-function table
    with pytest.raises(E.EngineError, match="has the target"):
        engine.set_sites_gauss(1, CLASS_MIX, *S.classes())
    # bh_evaluate_batch never reads the table
    S.register_mixed(engine)
    for a, b in zip(engine.evaluate_batch(nlay, h, vp, vs, noise, rho=rho), flat):
        assert np.array_equal(bits(a), bits(b))


# ---- chains ------------------------------------------------------------------------------------------------
NS, C, SEED, NRF, RCOND = 4, 3, 91, 60, 1e-5   # three chains per site: site boundaries fall inside a wavefront of the window kernels
INIT = dict(nchains=1, iter_burnin=150, iter_main=75, acceptance=(40, 80), thickmin=0.1, lvz=0.1, hvz=None, rcond=RCOND, maxmodels=15)
# the installed laws differ: the curve's correlation fixed at 0 with errors (scaled), without (nocorr), ranged (exp); the receiver
# function's fixed at 0.98 and 0.92 (Gauss, two classes), ranged (exp), and site 3 has none
SITE_PRIORS = [
    dict(PRIORS, swdnoise_corr=0., rfnoise_corr=0.98, layers=(1, 12)),
    dict(PRIORS, swdnoise_corr=0., rfnoise_corr=0.92, vs=(2.5, 4.5), z=(0, 50)),
    dict(PRIORS, swdnoise_corr=(0.1, 0.6), rfnoise_corr=(0.35, 0.75), rfnoise_sigma=(1e-4, 0.03)),
    dict(PRIORS, swdnoise_corr=0.),
]
WITH_YERR, LACKS_RF = (0,), (3,)
CHAIN_K = (21, 12, 30, 9)
CHAIN_LAWS = [[SCALED, GAUSS], [NOCORR, GAUSS], [EXP, EXP], [NOCORR, GAUSS]]   # (site 3's second entry: the descriptor's, not read)


def chain_slots(g, s, with_yerr=WITH_YERR, lacks=LACKS_RF):
    """site s: [Rayleigh phase at its own periods, P receiver function cut to its first 60 samples (one slab in every call)]"""
    rs = np.random.RandomState(900 + s)
    xs, ys = np.asarray(g["xsw"], dtype=float), np.asarray(g["ysw"], dtype=float)
    x1 = np.linspace(xs.min() + 0.3 * s, xs.max() - 1.1 * s, CHAIN_K[s])
    yerr = rs.uniform(0.01, 0.03, x1.size) if s in with_yerr else None
    t1 = bh.RayleighDispersionPhase(x1, np.interp(x1, xs, ys) + rs.normal(0, 0.02, x1.size), yerr=yerr)
    t2 = bh.PReceiverFunction(g["xrf"][:NRF], g["yrf"][:NRF] + rs.normal(0, 0.01, NRF))
    t2.moddata.plugin.set_modelparams(gauss=1.0, p=6.4)
    return [t1, None if s in lacks else t2]


@pytest.mark.parametrize("depth", [None, 1, 3])
def test_chains_walk_their_one_site_runs_under_their_own_laws(depth, tmp_path):
    g = golden("chain_golden.npz")
    names = ["st%d" % s for s in range(NS)]
    inits = [dict(INIT, savepath=str(tmp_path / "multi")) for _ in range(NS)]
    st = bh.SiteTargets([chain_slots(g, s) for s in range(NS)], names=names, per_site_x="all", per_site_rf=True, missing=True,
                        per_site_law=True)
    dc = DeviceChains(st, C, inits, SITE_PRIORS, seed=SEED, spec_depth=depth, search="reference").run()
    assert dc.prior_table and (dc.depth > 1 or depth == 1)
    assert np.array_equal(st.site_law_arrays(), CHAIN_LAWS)
    assert np.array_equal(st.gauss_class_arrays()[1][0], [0, 1, -1, -1])
    paths = dc.save() if depth is None else None
    for s in range(NS):
        ip = dict(INIT, savepath=str(tmp_path / "one" / names[s]), station=names[s])
        own = bh.JointTarget([t for t in chain_slots(g, s) if t is not None])
        one = DeviceChains(own, C, ip, SITE_PRIORS[s], seed=SEED, chain_offset=s * C, spec_depth=depth, search="reference").run()
        assert [LAW_CODES[t.law()] for t in own.targets] == CHAIN_LAWS[s][:1 if s in LACKS_RF else 2]   # what the sampler installed
        what = "depth %s site %d" % (depth, s)
        for phase in ("p1", "p2"):
            same_samples(dc.samples(phase, site=s), one.samples(phase), what + " " + phase)
        a, b = dc.state_host(), one.state_host()
        for k in ("proposed", "accepted", "propdist"):
            assert np.array_equal(a[k][:, s * C:(s + 1) * C], b[k]), "%s: %s" % (what, k)
        if paths is not None:
            dpath = one.save()
            files = sorted(f for f in os.listdir(dpath) if f.endswith(".npy"))
            assert files and files == sorted(f for f in os.listdir(paths[s]) if f.endswith(".npy"))
            for f in files:
                assert np.array_equal(np.load(os.path.join(dpath, f)), np.load(os.path.join(paths[s], f)), equal_nan=True), f
            assert os.path.exists(os.path.join(paths[s], "%s_config.pkl" % names[s]))


def test_one_law_at_every_site_equals_the_run_without_the_flag():
    g = golden("chain_golden.npz")
    priors = [dict(p, swdnoise_corr=0., rfnoise_corr=0.98) for p in SITE_PRIORS]
    runs = []
    for flag in (True, False):
        st = bh.SiteTargets([chain_slots(g, s, with_yerr=(), lacks=()) for s in range(NS)], per_site_x="all", per_site_rf=True,
                            missing=True, per_site_corr=True, per_site_law=flag)
        runs.append(DeviceChains(st, C, INIT, priors, seed=SEED, spec_depth=3, search="reference").run())
        assert np.array_equal(st.site_law_arrays(), [[NOCORR, GAUSS]] * NS) and st.per_site_law == flag
    for phase in ("p1", "p2"):
        same_samples(runs[0].samples(phase), runs[1].samples(phase), "one law " + phase)
    a, b = runs[0].state_host(), runs[1].state_host()
    for k in ("proposed", "accepted", "propdist"):
        assert np.array_equal(a[k], b[k]), k
