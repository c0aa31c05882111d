"""Sites with their own Gauss-law noise correlation on the MI355X (include/bh_engine_sites_gauss.h, SiteTargets(per_site_corr=True)).
The rule under test: a model of site s gets, on a Gauss-law target, what a call with site s's own R^-1 / ln|R| in the descriptor
gives it -- the bits of the existing contraction run on the same batch.  The reference is therefore the project's own existing
path (bh_sites_set without a class table), evaluated once per class over the WHOLE batch (same B, same n: same form and slabs);
no tolerance.  logL is checked against tests/like_ref.py within that module's own bound as well."""
import os

import numpy as np
import pytest

from conftest import golden
import bayhunter_amd as bh
import like_ref as LR
from bayhunter_amd import engine as E
from bayhunter_amd.device_chains import DeviceChains
from bayhunter_amd.synth import synth_models
from bayhunter_amd.Targets import Valuation
from test_gpu_like_paths import tuned
from test_gpu_sites import eval_device
from test_gpu_sites_x import PRIORS, bits

pytestmark = pytest.mark.gpu

PER = np.linspace(2.0, 60.0, 30)
RCOND = 1e-5
CLASS_CORR = (0.90, 0.94, 0.98, 0.96)
NSITES = 6
CLASS_OF = np.array([0, 1, 1, 2, 2, 0], dtype=np.int32)     # two pairs of sites share a class; with 4 classes class 3 has no site
_CLASSES = {}


def gauss_class(n, corr):
    """(R^-1, ln|R|) of a class: what Valuation.init_covariance_gauss leaves for a correlation fixed at `corr`"""
    if (n, corr) not in _CLASSES:
        v = Valuation()
        v.init_covariance_gauss(corr, n, rcond=RCOND)
        _CLASSES[(n, corr)] = (np.ascontiguousarray(v.corr_inv, dtype=np.float64), float(v.logcorr_det))
    return _CLASSES[(n, corr)]


def class_table(n, nclass):
    mats = [gauss_class(n, c) for c in CLASS_CORR[:nclass]]
    return np.stack([m[0] for m in mats]), np.array([m[1] for m in mats])


def structure(n):
    """a Rayleigh phase curve beside a P receiver function of n samples under the Gauss law (n = 1024: the receiver function alone)"""
    rf = dict(kind=E.TARGET_RF, law=E.LAW_GAUSS, n=n, waveno=0, p=6.4, gauss=2.5, tshift=5.0)
    if n > 512:
        return [dict(rf, nsamp=2048, fsamp=20.0)]
    return [dict(kind=E.TARGET_SWD, law=E.LAW_NOCORR, n=30, x=PER, iwave=2, igr=0), dict(rf, nsamp=512, fsamp=5.0)]


def site_descs(n, rs):
    """NSITES sites of one structure with observed data of their own; the Gauss-law target's matrix is filled in per class"""
    out = []
    for s in range(NSITES):
        ds = []
        for d in structure(n):
            d = dict(d)
            d["yobs"] = 3.0 + 0.02 * np.arange(30) + rs.normal(0, 0.05, 30) if d["kind"] == E.TARGET_SWD else rs.normal(0, 0.05, d["n"])
            ds.append(d)
        out.append(ds)
    return out


def with_class(ds, n, c):
    """descriptors ds with class c's matrix on the Gauss-law target"""
    out = [dict(d) for d in ds]
    out[-1]["rinv"], out[-1]["logdet_r"] = gauss_class(n, CLASS_CORR[c])
    return out


def site_rows(counts, bad_at):
    """The site of every row, built by hand: site s gets counts[s] rows, the sites' rows interleaved round robin; two rows, at the
    positions bad_at, are out of range (-1 and NSITES).  Returns (site for the device entry, site for the host entry -- which
    refuses a site out of range: those two rows go to site 5 there)."""
    left = list(counts)
    order = []
    while any(left):
        for s in range(NSITES):
            if left[s]:
                order.append(s)
                left[s] -= 1
    for pos, val in zip(bad_at, (-1, NSITES)):
        order.insert(pos, val)
    dev = np.array(order, dtype=np.int32)
    host = dev.copy()
    host[list(bad_at)] = 5
    return dev, host


# (n, B, rows per site, classes, forms to force): the classes receive 1 / 64 / 65 rows (B = 132: one row, a full 64-row tile, a
# tile and one row; one 128-row tile each when that form is forced), 1 / 129 / 168 (B = 300: past a 128-row tile by one row),
# 64 / 65 / 169 (B = 300 again: the 64-row boundaries with several K tiles and column tiles), 1 / 1024 / 1021 (B = 2048: the
# automatic choice is the 128 x 128 form with the K split: NSPLIT_AUTO)
CASES = {
    "n30": (30, 132, (1, 40, 24, 33, 32, 0), 4, (64, 128)),
    "n200": (200, 300, (1, 100, 29, 100, 68, 0), 4, (64, 128)),
    "n200b": (200, 300, (40, 33, 32, 100, 69, 24), 4, (64, 128)),
    "n1024": (1024, 2048, (1, 600, 424, 600, 421, 0), 3, (0,)),
}


# bh_gauss_nsplit(2048, 1024) (gauss_kernel.hip): 2 column halves x 8 column blocks x 4 K ranges in the 128 x 128 form; the 64 x 64
# form would take 16 slabs
NSPLIT_AUTO = {"n1024": 64}


def slab_count(B, n):
    import ctypes
    f = ctypes.CDLL(E.LIB_PATH)._Z15bh_gauss_nsplitii
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_int]
    return f(B, n)


def batch(rs, B, nt):
    nlay, h, vp, vs, rho = synth_models(rs, B, 10, ragged=True)
    if nt > 1:
        vs[0, ::11] = 9.0        # a few models whose dispersion fails
    noise = np.column_stack([rs.uniform(0.1, 0.6, B) if i % 2 == 0 else rs.uniform(0.02, 0.1, B) for i in range(2 * nt)])
    return nlay, h, vp, vs, rho, noise


def assert_rows(got, refs, cls, rows, what):
    """rows of `got` against the evaluation of their own class, bit for bit: logL, misfits, err and the synthetics"""
    for c in sorted(set(cls[rows])):
        m = np.zeros(len(cls), bool)
        m[rows] = True
        m &= cls == c
        for k, name in enumerate(("logL", "misfits", "err", "ymod")):
            assert np.array_equal(got[k][m], refs[c][k][m]), "%s: %s of class %d" % (what, name, c)


def run_case(eng, case, tile):
    n, B, counts, nclass, _ = CASES[case]
    rs = np.random.RandomState(1000 + n)
    descs = site_descs(n, rs)
    nt, tgt = len(descs[0]), len(descs[0]) - 1
    nlay, h, vp, vs, rho, noise = batch(rs, B, nt)
    models = (nlay, h, vp, vs, rho)
    site_d, site_h = site_rows(counts, (7, B - 5))
    assert site_d.size == B and np.array_equal(np.bincount(site_d[(site_d >= 0) & (site_d < NSITES)], minlength=NSITES), counts)
    rinv, logdet = class_table(n, nclass)
    yobs = np.vstack([np.concatenate([d["yobs"] for d in ds]) for ds in descs])
    cls_h, good = CLASS_OF[site_h], np.flatnonzero((site_d >= 0) & (site_d < NSITES))
    what = "%s tile %d" % (case, tile)
    with tuned(eng, "gauss_tile", tile):
        if tile == 0 and case in NSPLIT_AUTO:   # the automatic choice is the form the case is about
            assert slab_count(B, n) == NSPLIT_AUTO[case], what
        # the reference: the whole batch once per class through the existing sites path, that class's matrix in the descriptor
        refs = {}
        for c in sorted(set(CLASS_OF)):
            eng.set_targets(with_class(descs[0], n, c))
            eng.set_sites(yobs)
            refs[c] = eng.evaluate_sites(nlay, h, vp, vs, noise, site_h, rho=rho, want_ymod=True)
        # the class table
        eng.set_targets(with_class(descs[0], n, 0))
        eng.set_sites(yobs)
        eng.set_sites_gauss(tgt, CLASS_OF, rinv, logdet)
        got = eng.evaluate_sites(nlay, h, vp, vs, noise, site_h, rho=rho, want_ymod=True)
        assert_rows(got, refs, cls_h, np.arange(B), what + " host")
        again = eng.evaluate_sites(nlay, h, vp, vs, noise, site_h, rho=rho, want_ymod=True)
        for a, b in zip(got, again):        # the grouping's order does not show
            assert np.array_equal(bits(a), bits(b)), what + ": not repeatable"
        dgot = eval_device(eng, models, noise, site_d, eng.ldy)
        assert_rows(dgot, refs, cls_h, good, what + " device")
        dagain = eval_device(eng, models, noise, site_d, eng.ldy)
        for a, b in zip(dgot, dagain):
            assert np.array_equal(bits(a), bits(b)), what + ": device entry not repeatable"
        for k in (7, B - 5):                # a site out of range fails in band, as the existing path reports it
            assert dgot[2][k] == 1 and dgot[0][k] == -1e15 and np.all(dgot[1][k] == 1e15)
        # all sites in ONE class: the existing sites path, bit for bit
        eng.set_sites_gauss(tgt, np.zeros(NSITES, np.int32), rinv[:1], logdet[:1])
        one = eng.evaluate_sites(nlay, h, vp, vs, noise, site_h, rho=rho, want_ymod=True)
        for a, b in zip(one, refs[0]):
            assert np.array_equal(bits(a), bits(b)), what + ": one class against the path without a table"
        done = eval_device(eng, models, noise, site_d, eng.ldy)
        for a, b in zip(done, refs[0]):
            assert np.array_equal(bits(a[good]), bits(b[good])), what + ": one class, device entry"
    return descs, got, noise, site_h, n


def check_against_the_reference(descs, got, noise, site, n, what):
    """logL against the extended-precision reference with the site's data and its class's matrix, within like_ref's bound;
    another class's matrix lies far outside it"""
    logL, _, err, ymod = got
    for s in (1, 3):
        m = np.flatnonzero((site == s) & (err == 0))[:6]
        assert m.size
        c = int(CLASS_OF[s])
        ref, _, bound, _ = LR.joint_ref(with_class(descs[s], n, c), ymod[m], noise[m])
        LR.assert_within(logL[m], ref, bound, "%s site %d" % (what, s))
        other, _, _, _ = LR.joint_ref(with_class(descs[s], n, (c + 1) % 3), ymod[m], noise[m])
        assert np.all(np.abs(logL[m] - other.astype(float)) > 1e3 * bound)


@pytest.mark.parametrize("case,tile", [(c, t) for c in ("n30", "n200", "n200b", "n1024") for t in CASES[c][4]])
def test_every_model_gets_its_own_class_matrix(engine, case, tile):
    descs, got, noise, site, n = run_case(engine, case, tile)
    if any(d["kind"] == E.TARGET_SWD for d in descs[0]):
        assert (got[2] != 0).any()
    check_against_the_reference(descs, got, noise, site, n, "%s tile %d" % (case, tile))


@pytest.mark.parametrize("case", ["n30", "n200", "n1024"])
def test_in_kernel_matvec_with_classes(engine, case):
    """no_mfma (read when an engine is created): the likelihood kernel's own mat-vec reads the matrix of the model's class"""
    before = engine.tuning("no_mfma")
    engine.set_tuning("no_mfma", 1)
    eng = None
    try:
        eng = E.Engine(0)
        eng.set_swd_search("reference")
        eng.set_swd_arith("exact")
        descs, got, noise, site, n = run_case(eng, case, 0)
        check_against_the_reference(descs, got, noise, site, n, case + " no_mfma")
    finally:
        if eng is not None:
            eng.close()
        engine.set_tuning("no_mfma", before)


# ---- a Gauss-law slot that some site lacks -----------------------------------------------------------------
NRF = 60
M_PRESENT = np.array([[1, 1], [1, 0], [0, 1], [1, 1]], bool)     # [Rayleigh phase, P receiver function]
M_CLASS = np.array([0, -1, 1, 0], dtype=np.int32)
M_K = (30, 17, 0, 9)                                              # periods of every site


def missing_setup(rs):
    S = 4
    descs = []
    for s in range(S):
        k = M_K[s] or 30
        x = np.linspace(2.0 + s, 60.0 - 2 * s, k)
        d0 = dict(kind=E.TARGET_SWD, law=E.LAW_NOCORR, n=k, x=x, iwave=2, igr=0, yobs=3.0 + 0.02 * x + rs.normal(0, 0.05, k))
        d1 = dict(kind=E.TARGET_RF, law=E.LAW_GAUSS, n=NRF, waveno=0, p=6.4, gauss=2.5, tshift=5.0, nsamp=512, fsamp=5.0,
                  yobs=rs.normal(0, 0.05, NRF))
        if M_CLASS[s] >= 0:
            d1["rinv"], d1["logdet_r"] = gauss_class(NRF, CLASS_CORR[M_CLASS[s]])
        descs.append([d0, d1])
    cap = 30
    caps = [dict(descs[0][0], n=cap, x=np.ones(cap), yobs=np.zeros(cap)), dict(descs[0][1])]
    ldy = cap + NRF
    n = np.zeros((S, 2), np.int32)
    x, yobs = np.zeros((S, ldy)), np.zeros((S, ldy))
    for s in range(S):
        if M_PRESENT[s, 0]:
            k = descs[s][0]["n"]
            n[s, 0] = k
            x[s, :k], yobs[s, :k] = descs[s][0]["x"], descs[s][0]["yobs"]
        if M_PRESENT[s, 1]:
            n[s, 1] = NRF
            yobs[s, cap:] = descs[s][1]["yobs"]
    p = np.zeros((S, 2))
    p[M_PRESENT[:, 1], 1] = 6.4
    return descs, caps, n, x, yobs, p, np.zeros((S, 2)), cap


def test_a_gauss_slot_that_some_site_lacks(engine):
    """4 sites over [Rayleigh phase, P receiver function under the Gauss law]: one lacks the receiver function, one the curve, the
    others fall in two classes.  Every site equals its one-site call over the targets it has (reference search, n <= 64)."""
    rs = np.random.RandomState(31)
    descs, caps, n, x, yobs, p, nsv, cap = missing_setup(rs)
    B = 150
    nlay, h, vp, vs, rho, noise = batch(rs, B, 2)
    site = (np.arange(B) % 4).astype(np.int32)
    rinv, logdet = class_table(NRF, 2)
    engine.set_targets(caps)
    engine.set_sites_missing_gauss(n, x, yobs)
    engine.set_sites_rf(p, nsv)
    engine.set_sites_gauss(1, M_CLASS, rinv, logdet)
    got = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho, want_ymod=True)
    dgot = eval_device(engine, (nlay, h, vp, vs, rho), noise, site, engine.ldy)
    for a, b in zip(got, dgot):
        assert np.array_equal(bits(a), bits(b))
    for s in range(4):
        m = site == s
        have = np.flatnonzero(M_PRESENT[s])
        engine.set_targets([descs[s][t] for t in have])
        ncol = np.column_stack((2 * have, 2 * have + 1)).ravel()
        ref = engine.evaluate_batch(nlay, h, vp, vs, noise[:, ncol], rho=rho, want_ymod=True)
        assert np.array_equal(bits(got[0][m]), bits(ref[0][m])), "site %d: logL" % s
        assert np.array_equal(got[2][m], ref[2][m]), "site %d: err" % s
        ok = m & (ref[2] == 0)
        assert ok.any()
        o = 0
        for j, t in enumerate(have):
            k = n[s, t]
            lo = 0 if t == 0 else cap
            assert np.array_equal(bits(got[1][ok, t]), bits(ref[1][ok, j])), "site %d: misfit of slot %d" % (s, t)
            assert np.array_equal(bits(got[3][ok, lo:lo + k]), bits(ref[3][ok, o:o + k])), "site %d: synthetics of slot %d" % (s, t)
            o += k
        assert np.array_equal(bits(got[1][ok, 2]), bits(ref[1][ok, len(have)])), "site %d: joint misfit" % s
        for t in np.flatnonzero(~M_PRESENT[s]):         # the absent slot: misfit 0, synthetics zeros
            lo, hi = (0, cap) if t == 0 else (cap, cap + NRF)
            assert np.all(got[1][m, t] == 0.0) and np.all(bits(got[3][m, lo:hi]) == 0)


# ---- entry points ------------------------------------------------------------------------------------------
def test_entry_point_refusals_and_the_tables_lifetime(engine):
    rs = np.random.RandomState(5)
    n = 30
    descs = site_descs(n, rs)
    yobs = np.vstack([np.concatenate([d["yobs"] for d in ds]) for ds in descs])
    rinv, logdet = class_table(n, 3)
    L, hd = engine._L, engine._h
    P = lambda a: a.ctypes.data
    cls = CLASS_OF.copy()

    def rc(target=1, nsites=NSITES, nclass=3, c=cls, r=rinv, ld=logdet):
        c = None if c is None else np.ascontiguousarray(c, dtype=np.int32)
        return L.bh_sites_set_gauss(hd, target, nsites, nclass, None if c is None else P(c), None if r is None else P(r),
                                    None if ld is None else P(ld))

    engine.set_targets(with_class(descs[0], n, 0))
    assert rc() == E.BH_EINVAL and b"no site table" in L.bh_engine_last_error(hd)
    engine.set_sites(yobs)
    assert rc() == E.BH_OK
    assert rc(nsites=NSITES - 1) == E.BH_EINVAL
    assert rc(target=0) == E.BH_EINVAL and b"BH_LAW_GAUSS" in L.bh_engine_last_error(hd)     # the dispersion target: not Gauss
    assert rc(target=2) == E.BH_EINVAL and rc(target=-1) == E.BH_EINVAL
    assert rc(nclass=0) == E.BH_EINVAL
    for bad in (3, -2):
        b = cls.copy()
        b[4] = bad
        assert rc(c=b) == E.BH_EINVAL
    b = cls.copy()
    b[2] = -1                               # bh_sites_set: every site has every target
    assert rc(c=b) == E.BH_EINVAL and b"has the target" in L.bh_engine_last_error(hd)
    for val in (np.nan, np.inf):
        r = rinv.copy()
        r[2, 5, 7] = val
        assert rc(r=r) == E.BH_EINVAL
        ld = logdet.copy()
        ld[1] = val
        assert rc(ld=ld) == E.BH_EINVAL
    assert rc(c=None) == E.BH_EINVAL and rc(r=None) == E.BH_EINVAL and rc(ld=None) == E.BH_EINVAL
    # above BH_SITES_GAUSS_MAXBYTES (1 GiB): refused before the arrays are read (these are not that long)
    too_many = (1 << 30) // (8 * n * n) + 1
    assert rc(nclass=too_many) == E.BH_EUNSUPPORTED and b"BH_SITES_GAUSS_MAXBYTES" in L.bh_engine_last_error(hd)
    assert rc(nclass=4097) == E.BH_EUNSUPPORTED and b"BH_SITES_GAUSS_MAXCLASSES" in L.bh_engine_last_error(hd)

    # lifetime: bh_sites_set and bh_targets_set drop the table -- the descriptor's matrix serves every site again
    nlay, h, vp, vs, rho, noise = batch(rs, 40, 2)
    site = (np.arange(40) % NSITES).astype(np.int32)
    tabled = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho)       # (a refused call leaves the table in force alone)
    engine.set_sites(yobs)
    plain = engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho)
    other = (CLASS_OF[site] != 0) & (plain[2] == 0)
    assert other.any() and np.array_equal(plain[2], tabled[2])
    assert np.array_equal(bits(tabled[0][~other]), bits(plain[0][~other])) and np.all(tabled[0][other] != plain[0][other])
    assert rc() == E.BH_OK
    engine.set_sites(yobs)
    assert np.array_equal(bits(engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho)[0]), bits(plain[0]))
    assert rc() == E.BH_OK
    engine.set_targets(with_class(descs[0], n, 0))
    engine.set_sites(yobs)
    assert np.array_equal(bits(engine.evaluate_sites(nlay, h, vp, vs, noise, site, rho=rho)[0]), bits(plain[0]))
    assert rc() == E.BH_OK                 # bh_evaluate_batch never reads it
    engine.set_targets(with_class(descs[0], n, 0))
    ref = engine.evaluate_batch(nlay, h, vp, vs, noise, rho=rho)
    engine.set_sites(yobs)
    assert rc() == E.BH_OK
    assert np.array_equal(bits(engine.evaluate_batch(nlay, h, vp, vs, noise, rho=rho)[0]), bits(ref[0]))

    # a Gauss-law slot that a site lacks: bh_sites_set_missing refuses, its sibling accepts and then needs the class table
    mdescs, caps, cnt, x, myobs, p, nsv, cap = missing_setup(rs)
    engine.set_targets(caps)
    args = (hd, 4, P(cnt), P(x), P(myobs), None)
    assert L.bh_sites_set_missing(*args) == E.BH_EUNSUPPORTED
    assert L.bh_sites_set_missing_gauss(*args) == E.BH_OK
    engine.nsites = 4
    engine.set_sites_rf(p, nsv)
    site4 = (np.arange(40) % 4).astype(np.int32)
    with pytest.raises(E.EngineError, match="bh_sites_set_gauss"):
        engine.evaluate_sites(nlay, h, vp, vs, noise, site4, rho=rho)
    mr, ml = class_table(NRF, 2)
    for wrong in ([0, 0, 1, 0], [0, -1, -1, 0]):          # a class where the count is 0; -1 where the site has the target
        with pytest.raises(E.EngineError, match="bh_sites_set_gauss"):
            engine.set_sites_gauss(1, wrong, mr, ml)
    engine.set_sites_gauss(1, M_CLASS, mr, ml)
    assert np.all(engine.evaluate_sites(nlay, h, vp, vs, noise, site4, rho=rho)[2][site4 == 2] == 0)
    engine.set_sites_rf(p, nsv)             # ... which every bh_sites_set* drops
    with pytest.raises(E.EngineError, match="bh_sites_set_gauss"):
        engine.evaluate_sites(nlay, h, vp, vs, noise, site4, rho=rho)


# ---- chains ------------------------------------------------------------------------------------------------
S, C, SEED = 4, 3, 77       # three chains per site: site boundaries fall inside a wavefront of the window kernels
CORR = (0.90, 0.94, 0.94, 0.98)
INIT = dict(nchains=1, iter_burnin=150, iter_main=75, acceptance=(40, 80), thickmin=0.1, lvz=0.1, hvz=None, rcond=RCOND, maxmodels=15)
SITE_PRIORS = [
    dict(PRIORS, rfnoise_corr=CORR[0], layers=(1, 12)),
    dict(PRIORS, rfnoise_corr=CORR[1], vs=(2.5, 4.5), z=(0, 50)),
    dict(PRIORS, rfnoise_corr=CORR[2], rfnoise_sigma=(1e-4, 0.03)),
    dict(PRIORS, rfnoise_corr=CORR[3]),
]
LACKS_RF = 0                # so that sites 1 and 2, both at 0.94, share a class
CHAIN_K = (21, 12, 30, 9)


def chain_slots(g, s, lacks=LACKS_RF):
    """site s: [Rayleigh phase at its own periods, P receiver function cut to its first 60 samples (nsplit = 1 in every call)]"""
    rs = np.random.RandomState(700 + s)
    xs, ys = np.asarray(g["xsw"], dtype=float), np.asarray(g["ysw"], dtype=float)
    x1 = np.linspace(xs.min() + 0.3 * s, xs.max() - 1.1 * s, CHAIN_K[s])
    t1 = bh.RayleighDispersionPhase(x1, np.interp(x1, xs, ys) + rs.normal(0, 0.02, x1.size))
    t2 = bh.PReceiverFunction(g["xrf"][:NRF], g["yrf"][:NRF] + rs.normal(0, 0.01, NRF))
    t2.moddata.plugin.set_modelparams(gauss=1.0, p=6.4)
    return [t1, None if s == lacks else t2]


def own_targets(g, s, lacks=LACKS_RF):
    return bh.JointTarget([t for t in chain_slots(g, s, lacks) if t is not None])


def same_samples(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=True), "%s: %s" % (what, k)


@pytest.mark.parametrize("depth", [None, 1, 3])
def test_chains_walk_their_one_site_runs_under_their_own_correlation(depth, tmp_path):
    g = golden("chain_golden.npz")
    names = ["st%d" % s for s in range(S)]
    inits = [dict(INIT, savepath=str(tmp_path / "multi")) for _ in range(S)]
    st = bh.SiteTargets([chain_slots(g, s) for s in range(S)], names=names, per_site_x="all", per_site_rf=True, missing=True,
                        per_site_corr=True)
    dc = DeviceChains(st, C, inits, SITE_PRIORS, seed=SEED, spec_depth=depth, search="reference").run()
    assert dc.prior_table and (dc.depth > 1 or depth == 1)
    class_of = st.gauss_class_arrays()[1][0]
    assert np.array_equal(class_of, [-1, 0, 0, 1])
    paths = dc.save() if depth is None else None
    for s in range(S):
        ip = dict(INIT, savepath=str(tmp_path / "one" / names[s]), station=names[s])
        one = DeviceChains(own_targets(g, s), C, ip, SITE_PRIORS[s], seed=SEED, chain_offset=s * C, spec_depth=depth,
                           search="reference").run()
        assert not one.prior_table
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


def test_one_correlation_at_every_site_equals_the_run_without_the_flag():
    g = golden("chain_golden.npz")
    priors = [dict(p, rfnoise_corr=0.98) for p in SITE_PRIORS]
    runs = []
    for flag in (True, False):
        st = bh.SiteTargets([chain_slots(g, s, lacks=None) for s in range(S)], per_site_x="all", per_site_rf=True, per_site_corr=flag)
        runs.append(DeviceChains(st, C, INIT, priors, seed=SEED, spec_depth=3, search="reference").run())
        tables = st.gauss_class_arrays()
        assert np.array_equal(tables[1][0], [0, 0, 0, 0]) and tables[1][1].shape[0] == 1
    for phase in ("p1", "p2"):
        same_samples(runs[0].samples(phase), runs[1].samples(phase), "one class " + phase)
