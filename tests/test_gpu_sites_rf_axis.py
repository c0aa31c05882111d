"""A receiver-function time axis and Gauss filter per site on the MI355X (include/bh_engine_sites_rf_axis.h,
SiteTargets(per_site_rf="all")).  The rule under test: a model of site s gets, on a receiver-function target, what a one-site call
gives whose descriptor holds site s's nsamp, fsamp, tshift, gauss and n -- trace, failure behaviour, logL and misfits bit for bit,
the trace followed by exact zeros up to the capacity of its columns.  The reference is therefore the project's own one-site path
(bh_evaluate_batch), no tolerance; traces against tests/rf_ref.py at the project's bar (1e-9 of the peak), the Gauss law's logL
against tests/like_ref.py within that module's own bound.

Gauss law, capacity above 64 (test_gauss_law_capacity_200): the parent has no path that gives a site of FEWER samples than the
capacity its own n-dependent terms (n ln 2 pi, 2 n ln sigma, the misfit's 1/n), so the existing class contraction run on the same
batch with the embedded matrices is compared bit for bit on the rows of the sites whose count IS the capacity; every row, the
shorter sites' included, is held to like_ref's bound of the truth."""
import os
import pickle

import numpy as np
import pytest

import bayhunter_amd as bh
import like_ref as LR
import rf_ref as RR
from bayhunter_amd import engine as E
from bayhunter_amd.device_chains import DeviceChains
from bayhunter_amd.synth import synth_models
from bayhunter_amd.Targets import Valuation
from test_gpu_like_paths import tuned
from test_gpu_sites import eval_device
from test_gpu_sites_rf import bits, models

pytestmark = pytest.mark.gpu

# (nsamp, n, fsamp Hz, tshift s, gauss).  The spectral cut sits on both sides of its boundary: jc = 32 = nsamp / 2 at 64 / 4 Hz /
# 1.0 (inactive, the Nyquist bin kept), 51 at 256 / 10 Hz / 1.0, 510 > 256 at 512 / 5 Hz / 2.5, 255 < 256 at 512 / 20 Hz / 5.0;
# active at 2048 / 20 Hz / 2.5 (510 of 1025 bins).  64: the second twiddle table has one entry; 128: its boundary; 65: odd, one
# past a wavefront; 512 / 512: every sample kept (no Python target gives it: 2 n <= nsamp there); 2048: the table's LDS request.
AXES = [(64, 30, 4.0, 2.0, 1.0), (128, 64, 5.0, 0.0, 2.5), (256, 65, 10.0, 5.0, 1.0), (512, 201, 5.0, 5.0, 2.5),
        (512, 512, 20.0, 10.0, 5.0), (2048, 1000, 20.0, 7.5, 2.5)]
SITE_P = np.array([4.0, 5.5, 6.4, 7.5, 9.0, 8.0])
SITE_NSV = np.array([0.0, 2.0, 0.0, 1.5, 0.0, 3.0])
PER = np.linspace(3.0, 40.0, 12)


def last_error(eng):
    return eng._L.bh_engine_last_error(eng._h).decode()


def rf_desc(law, waveno, axis, p, nsv, rs):
    nsamp, n, fsamp, tshift, gauss = axis
    return dict(kind=E.TARGET_RF, law=law, n=n, waveno=waveno, nsamp=nsamp, p=float(p), gauss=gauss, fsamp=fsamp, tshift=tshift,
                nsv=float(nsv), yobs=rs.normal(0, 0.05, n))


def swd_desc(rs):
    return dict(kind=E.TARGET_SWD, law=E.LAW_NOCORR, n=12, x=PER, iwave=2, igr=0, yobs=3.0 + 0.02 * np.arange(12) + rs.normal(0, 0.05, 12))


def site_descs(case, rs, axes=AXES):
    """every site's own descriptors (None: the site lacks the slot).  A second receiver function of a site takes the NEXT axis of
    the list and a ray parameter 0.25 s/deg larger, so that a wrong table column shows."""
    S = len(axes)
    out = []
    for s in range(S):
        a0, a1 = axes[s], axes[(s + 1) % S]
        p, nsv = SITE_P[s], SITE_NSV[s]
        if case == "exp_P":
            ds = [rf_desc(E.LAW_EXP, 0, a0, p, nsv, rs)]
        elif case == "nocorr_SV":
            ds = [rf_desc(E.LAW_NOCORR, 1, a0, p, nsv, rs), rf_desc(E.LAW_EXP, 0, a1, p + 0.25, nsv, rs)]
        elif case == "joint":
            ds = [swd_desc(rs), rf_desc(E.LAW_EXP, 0, a0, p, nsv, rs), rf_desc(E.LAW_NOCORR, 1, a1, p + 0.25, nsv, rs)]
        elif case == "lacks":
            ds = [swd_desc(rs), None if s == 2 else rf_desc(E.LAW_EXP, 0, a0, p, nsv, rs)]
        else:
            raise KeyError(case)
        out.append(ds)
    return out


def layout(descs):
    """(counts[S, nt], capacity[nt], column offsets[nt + 1]) of site descriptors"""
    n = np.array([[0 if d is None else d["n"] for d in ds] for ds in descs], dtype=np.int32)
    cap = n.max(axis=0)
    return n, cap, np.concatenate([[0], np.cumsum(cap)]).astype(int)


def capacity_descs(descs):
    """every slot's descriptor at the first site that has it, with the capacity as n and placeholders the site path never reads"""
    n, cap, _ = layout(descs)
    out = []
    for t in range(n.shape[1]):
        d = dict(next(ds[t] for ds in descs if ds[t] is not None))
        d["n"], d["yobs"] = int(cap[t]), np.zeros(cap[t])
        if d["kind"] == E.TARGET_SWD:
            d["x"] = np.ones(cap[t])
        else:
            d["nsamp"] = max(ds[t]["nsamp"] for ds in descs if ds[t] is not None)
            d.update(fsamp=1.0, tshift=0.0, gauss=1.0, p=1.0, nsv=0.0)
            if d["law"] == E.LAW_GAUSS:
                d["rinv"], d["logdet_r"] = np.eye(cap[t]), 0.0
        out.append(d)
    return out


def tables(descs):
    """the arrays of bh_sites_set_axes, bh_sites_set_rf and bh_sites_set_rf_axis"""
    n, cap, off = layout(descs)
    S, nt = n.shape
    x, yobs = np.zeros((S, off[-1])), np.zeros((S, off[-1]))
    p, nsv = np.zeros((S, nt)), np.zeros((S, nt))
    nsamp = np.full((S, nt), 4, np.int32)
    fsamp, tshift, gauss = np.ones((S, nt)), np.zeros((S, nt)), np.ones((S, nt))
    for s, ds in enumerate(descs):
        for t, d in enumerate(ds):
            if d is None:
                continue
            yobs[s, off[t]:off[t] + d["n"]] = d["yobs"]
            if d["kind"] == E.TARGET_SWD:
                x[s, off[t]:off[t] + d["n"]] = d["x"]
            else:
                p[s, t], nsv[s, t] = d["p"], d["nsv"]
                nsamp[s, t], fsamp[s, t], tshift[s, t], gauss[s, t] = d["nsamp"], d["fsamp"], d["tshift"], d["gauss"]
    return dict(n=n, x=x, yobs=yobs, p=p, nsv=nsv, nsamp=nsamp, fsamp=fsamp, tshift=tshift, gauss=gauss)


def register(eng, descs, classes=None):
    T = tables(descs)
    eng.set_targets(capacity_descs(descs))
    eng.set_sites_axes(T["n"], T["x"], T["yobs"])
    eng.set_sites_rf(T["p"], T["nsv"])
    eng.set_sites_rf_axis(T["nsamp"], T["fsamp"], T["tshift"], T["gauss"])
    for t, (class_of, rinv, logdet) in sorted((classes or {}).items()):
        eng.set_sites_gauss(t, class_of, rinv, logdet)
    return T


def one_site_calls(eng, descs, mods, noise):
    """every model through bh_evaluate_batch with each site's own descriptors (the whole batch: the same B), the noise columns
    those of the slots the site has"""
    out = []
    for ds in descs:
        have = [t for t, d in enumerate(ds) if d is not None]
        eng.set_targets([ds[t] for t in have])
        cols = np.array([c for t in have for c in (2 * t, 2 * t + 1)])
        out.append(eng.evaluate_batch(*mods[:4], noise[:, cols], rho=mods[4], want_ymod=True))
    return out


def assert_rule(got, refs, descs, site, rows, what):
    """rows of a mixed call against their site's one-site call: logL, err, the misfits of the slots the site has (0 in the others),
    the first n_s columns of every trace and exact zeros up to the capacity"""
    n, cap, off = layout(descs)
    nt = n.shape[1]
    logL, misf, err, ymod = got
    for s, (rl, rm, re_, ry) in enumerate(refs):
        m = np.zeros(len(site), bool)
        m[rows] = True
        m &= site == s
        assert m.any(), "%s: no row of site %d" % (what, s)
        have = [t for t in range(nt) if n[s, t] > 0]
        assert np.array_equal(bits(logL[m]), bits(rl[m])), "%s: logL of site %d" % (what, s)
        assert np.array_equal(err[m], re_[m]), "%s: err of site %d" % (what, s)
        assert np.array_equal(bits(misf[m][:, have + [nt]]), bits(rm[m])), "%s: misfits of site %d" % (what, s)
        ok = m & (err == 0)
        o = 0
        for t in range(nt):
            k = n[s, t]
            if k:
                assert np.array_equal(bits(ymod[ok, off[t]:off[t] + k]), bits(ry[ok, o:o + k])), "%s: slot %d of site %d" % (what, t, s)
                o += k
            else:
                assert np.all(misf[ok, t] == 0.0), "%s: misfit of the slot site %d lacks" % (what, s)
            tail = ymod[ok, off[t] + k:off[t + 1]]
            assert np.array_equal(bits(tail), np.zeros(tail.shape, np.int64)), "%s: zeros behind slot %d of site %d" % (what, t, s)


def site_rows(rs, B, S, bad_at):
    """the sites interleaved at random, every site present; for the device entry the rows bad_at are out of range (-1 and S)"""
    host = rs.randint(0, S, B).astype(np.int32)
    host[rs.permutation(B)[:S]] = np.arange(S)
    dev = host.copy()
    dev[list(bad_at)] = (-1, S)
    return host, dev


# Lmax 8 / 21 / 40: rf_coef_layers_sites_kernel<16> / <32> / rf_coef_sites_kernel of the site-axis builds; "joint" at 12 / 24: the
# _small builds behind the start gate, with the LDS floor; "lacks": site 2 has no trace (its workgroups write zeros and leave).
@pytest.mark.parametrize("case,Lmax", [("exp_P", 8), ("nocorr_SV", 21), ("exp_P", 40), ("joint", 12), ("joint", 24), ("lacks", 12)])
def test_each_site_equals_its_own_one_site_call(engine, case, Lmax):
    rs = np.random.RandomState(Lmax + 7 * len(case))
    descs = site_descs(case, rs)
    S, nt, B = len(descs), len(descs[0]), 150
    mods = models(rs, B, Lmax)
    noise = np.column_stack([rs.uniform(0.1, 0.6, B) if i % 2 == 0 else rs.uniform(0.02, 0.1, B) for i in range(2 * nt)])
    bad_at = (7, B - 5)
    host, dev = site_rows(rs, B, S, bad_at)
    refs = one_site_calls(engine, descs, mods, noise)
    register(engine, descs)
    got = engine.evaluate_sites(*mods[:4], noise, host, rho=mods[4], want_ymod=True)
    assert_rule(got, refs, descs, host, np.arange(B), "%s Lmax %d host" % (case, Lmax))
    dgot = eval_device(engine, mods, noise, dev, engine.ldy)
    good = np.setdiff1d(np.arange(B), bad_at)
    assert_rule(dgot, refs, descs, dev, good, "%s Lmax %d device" % (case, Lmax))
    for k in bad_at:                         # a site out of range fails in band
        assert dgot[2][k] == 1 and dgot[0][k] == -1e15
    assert (got[2] == 0).sum() > B // 2
    # two sites' traces differ: the first 64 samples of the models at site 1's axis and at site 3's
    t = 1 if descs[0][0]["kind"] == E.TARGET_SWD else 0
    o1, o3 = sum(d["n"] for d in descs[1][:t]), sum(d["n"] for d in descs[3][:t])
    both = (refs[1][2] == 0) & (refs[3][2] == 0)
    assert both.any() and not np.array_equal(refs[1][3][both, o1:o1 + 64], refs[3][3][both, o3:o3 + 64])


@pytest.mark.parametrize("switch,value", [("rf_no_cut", 1), ("rf_waves", 3), ("rf_threads", 128), ("rf_no_rot", 1), ("rf_no_realc", 1)])
def test_launch_switches_reach_the_site_axis_builds(engine, switch, value):
    """the experiment switches of bh_launch_rf (bh_tuning.h) in the site-axis launcher: with one set, every site still equals its
    one-site call made under the same switch -- rf_no_cut replaces every site's own jcut at launch, rf_waves / rf_threads pick
    the other build and workgroup size"""
    rs = np.random.RandomState(31)
    descs = site_descs("exp_P", rs, AXES[:4])
    S, B = len(descs), 40
    mods = models(rs, B, 10)
    noise = np.column_stack([rs.uniform(0.1, 0.6, B), rs.uniform(0.02, 0.1, B)])
    site, _ = site_rows(rs, B, S, (3, B - 2))
    with tuned(engine, switch, value):
        refs = one_site_calls(engine, descs, mods, noise)
        register(engine, descs)
        got = engine.evaluate_sites(*mods[:4], noise, site, rho=mods[4], want_ymod=True)
    assert_rule(got, refs, descs, site, np.arange(B), "%s = %d" % (switch, value))
    if switch == "rf_no_cut":       # the cut is active at site 2 (51 of 128 bins) and changes the last bits there
        refs_cut = one_site_calls(engine, descs, mods, noise)
        ok = (refs[2][2] == 0) & (refs_cut[2][2] == 0)
        assert not np.array_equal(refs[2][3][ok], refs_cut[2][3][ok])


def test_largest_trace_beside_the_shortest(engine):
    """nsamp 16384 (8000 samples: 134 KB of LDS for every workgroup of the launch, beyond the default dynamic limit) beside nsamp 64"""
    rs = np.random.RandomState(16384)
    descs = [[rf_desc(E.LAW_EXP, 0, (16384, 8000, 20.0, 10.0, 2.5), 6.4, 0.0, rs)], [rf_desc(E.LAW_EXP, 0, AXES[0], 7.0, 0.0, rs)]]
    B = 12
    mods = models(rs, B, 10)
    noise = np.tile([0.4, 0.05], (B, 1))
    site = (np.arange(B) % 2).astype(np.int32)
    refs = one_site_calls(engine, descs, mods, noise)
    register(engine, descs)
    got = engine.evaluate_sites(*mods[:4], noise, site, rho=mods[4], want_ymod=True)
    assert_rule(got, refs, descs, site, np.arange(B), "16384 beside 64")
    assert (got[2] == 0).any()


def test_site_traces_against_the_reference(engine):
    """two sites of different axes, P and SV, 24 models at each: 1e-9 of the peak against tests/rf_ref.py; every model finite"""
    rs = np.random.RandomState(21)
    nlay, h, vp, vs, rho = synth_models(rs, 24, 10, ragged=True)
    axes = [AXES[2], AXES[5]]
    descs = [[rf_desc(E.LAW_NOCORR, 0, a, p, nsv, rs), rf_desc(E.LAW_NOCORR, 1, a, p + 0.25, nsv, rs)]
             for a, p, nsv in zip(axes, (6.4, 8.75), (0.0, 1.5))]
    two = lambda a: np.concatenate([a, a], axis=-1)
    mods = (two(nlay), two(h), two(vp), two(vs), two(rho))
    site = np.repeat([0, 1], 24).astype(np.int32)
    noise = np.tile([0.0, 0.05, 0.0, 0.05], (48, 1))
    register(engine, descs)
    _, _, err, ymod = engine.evaluate_sites(*mods[:4], noise, site, rho=mods[4], want_ymod=True)
    assert np.all(err == 0)
    _, cap, off = layout(descs)
    for s, ds in enumerate(descs):
        for t, d in enumerate(ds):
            ref = RR.rf_ref(nlay, h, vp, vs, rho, d["p"], d["gauss"], d["nsamp"], d["fsamp"], d["tshift"], d["waveno"], d["n"], nsv=d["nsv"])
            want = np.asarray(ref.rf, dtype=np.float64)
            got = ymod[site == s, off[t]:off[t] + d["n"]]
            assert np.all(np.isfinite(want)) and np.all(np.isfinite(got))
            peak = np.max(np.abs(want))
            dev = np.max(np.abs(got - want)) / peak
            print("site %d wave %d: max deviation %.3e of the peak" % (s, d["waveno"], dev))
            assert dev <= 1e-9, (s, d["waveno"], dev)


# ---- Gauss law ---------------------------------------------------------------------------------------------
_CLASSES = {}


def gauss_class(n, corr):
    if (n, corr) not in _CLASSES:
        v = Valuation()
        v.init_covariance_gauss(corr, n, rcond=1e-5)
        _CLASSES[(n, corr)] = (np.ascontiguousarray(v.corr_inv, dtype=np.float64), float(v.logcorr_det))
    return _CLASSES[(n, corr)]


def gauss_sites(spec, rs):
    """spec: per site (axis, corr) or None (the site lacks the trace); [Rayleigh phase, P receiver function under the Gauss law]"""
    descs = []
    for s, sp in enumerate(spec):
        ds = [swd_desc(rs), None]
        if sp is not None:
            d = rf_desc(E.LAW_GAUSS, 0, sp[0], 5.0 + 0.5 * s, 0.0, rs)
            d["rinv"], d["logdet_r"] = gauss_class(d["n"], sp[1])
            ds[1] = d
        descs.append(ds)
    return descs


def padded_classes(spec, cap):
    """(class_of, rinv[nclass, cap, cap], logdet): a site's matrix in the top-left corner of a zero matrix, one class per (corr, n)"""
    keys, class_of = [], []
    for sp in spec:
        if sp is None:
            class_of.append(-1)
            continue
        k = (sp[0][1], sp[1])
        if k not in keys:
            keys.append(k)
        class_of.append(keys.index(k))
    rinv = np.zeros((len(keys), cap, cap))
    for c, (n, corr) in enumerate(keys):
        rinv[c, :n, :n] = gauss_class(n, corr)[0]
    return np.array(class_of, np.int32), rinv, np.array([gauss_class(n, corr)[1] for n, corr in keys])


def test_gauss_law_capacity_64(engine):
    """n = 40 / 60 / 64 in columns of 64: one form, one slab, partial tiles zero-filled -- the padded contraction adds exact zeros
    in the one-site call's order, so every site equals its one-site call of the same B bit for bit"""
    rs = np.random.RandomState(64)
    spec = [((128, 40, 5.0, 2.0, 1.0), 0.90), ((128, 60, 5.0, 0.0, 2.5), 0.94), ((128, 64, 10.0, 1.0, 2.5), 0.98),
            ((128, 60, 4.0, 3.0, 1.0), 0.94), None]
    descs = gauss_sites(spec, rs)
    S, B = len(descs), 132
    class_of, rinv, logdet = padded_classes(spec, 64)
    assert np.array_equal(class_of, [0, 1, 2, 1, -1]) and rinv.shape == (3, 64, 64)      # sites 1 and 3 share a class
    mods = models(rs, B, 10)
    noise = np.column_stack([rs.uniform(0.1, 0.6, B) if i % 2 == 0 else rs.uniform(0.02, 0.1, B) for i in range(4)])
    host, dev = site_rows(rs, B, S, (7, B - 5))
    refs = one_site_calls(engine, descs, mods, noise)
    register(engine, descs, {1: (class_of, rinv, logdet)})
    got = engine.evaluate_sites(*mods[:4], noise, host, rho=mods[4], want_ymod=True)
    assert_rule(got, refs, descs, host, np.arange(B), "capacity 64 host")
    dgot = eval_device(engine, mods, noise, dev, engine.ldy)
    assert_rule(dgot, refs, descs, dev, np.setdiff1d(np.arange(B), (7, B - 5)), "capacity 64 device")
    assert (got[2] == 0).sum() > B // 2


@pytest.mark.parametrize("tile", [64, 128])
def test_gauss_law_capacity_200(engine, tile):
    """n = 100 / 200 in columns of 200, B = 300, both contraction forms: nsplit and the form follow (B, capacity).  The rows of the
    sites of 200 samples equal the existing class contraction run on the same batch with the same embedded matrices and
    zero-padded data, bit for bit; every row lies within like_ref's bound of the truth formed with its own site's n, data and
    matrix, and another class's matrix far outside it."""
    rs = np.random.RandomState(200)
    long_, short = (512, 200, 5.0, 5.0, 2.5), (256, 100, 5.0, 5.0, 2.5)
    spec = [(short, 0.90), (long_, 0.94), (short, 0.98), (long_, 0.90)]
    descs = gauss_sites(spec, rs)
    S, B = len(descs), 300
    class_of, rinv, logdet = padded_classes(spec, 200)
    assert np.array_equal(class_of, [0, 1, 2, 3])
    mods = models(rs, B, 10)
    noise = np.column_stack([rs.uniform(0.1, 0.6, B) if i % 2 == 0 else rs.uniform(0.02, 0.1, B) for i in range(4)])
    site, _ = site_rows(rs, B, S, (7, B - 5))
    with tuned(engine, "gauss_tile", tile):
        T = register(engine, descs, {1: (class_of, rinv, logdet)})
        got = engine.evaluate_sites(*mods[:4], noise, site, rho=mods[4], want_ymod=True)
        # the existing class path: one shared axis (the long sites'), counts of 200 everywhere, the same tables otherwise
        shared = capacity_descs(descs)
        shared[1].update(nsamp=long_[0], fsamp=long_[2], tshift=long_[3], gauss=long_[4])
        engine.set_targets(shared)
        n200 = T["n"].copy()
        n200[:, 1] = 200
        engine.set_sites_missing_gauss(n200, T["x"], T["yobs"])
        engine.set_sites_rf(T["p"], T["nsv"])
        engine.set_sites_gauss(1, class_of, rinv, logdet)
        ref = engine.evaluate_sites(*mods[:4], noise, site, rho=mods[4], want_ymod=True)
    m = (site == 1) | (site == 3)
    for a, b, name in zip(got, ref, ("logL", "misfits", "err", "ymod")):
        assert np.array_equal(bits(a[m]), bits(b[m])), "tile %d: %s of the sites of 200 samples" % (tile, name)
    logL, _, err, ymod = got
    for s in range(S):
        r = np.flatnonzero((site == s) & (err == 0))[:6]
        assert r.size
        own = [descs[s][0], descs[s][1]]
        k = own[1]["n"]
        ym = np.hstack([ymod[r, :12], ymod[r, 12:12 + k]])
        want, _, bound, _ = LR.joint_ref(own, ym, noise[r])
        LR.assert_within(logL[r], want, bound, "tile %d site %d" % (tile, s))
        other = [own[0], dict(own[1])]
        other[1]["rinv"], other[1]["logdet_r"] = gauss_class(k, 0.96)
        wrong, _, _, _ = LR.joint_ref(other, ym, noise[r])
        assert np.all(np.abs(logL[r] - wrong.astype(float)) > 1e3 * bound)


# ---- API ---------------------------------------------------------------------------------------------------
def test_api_refusals_and_lifetime(engine):
    rs = np.random.RandomState(4)
    descs = site_descs("joint", rs, AXES[:4])
    S, nt, B = len(descs), 3, 40
    mods = models(rs, B, 10)
    noise = np.tile([0.0, 0.05, 0.4, 0.05, 0.0, 0.05], (B, 1))
    site = rs.randint(0, S, B).astype(np.int32)
    T = tables(descs)
    L, h = engine._L, engine._h
    P = lambda a: a.ctypes.data
    axis = lambda **kw: [P(np.ascontiguousarray(kw.get(k, T[k]))) for k in ("nsamp", "fsamp", "tshift", "gauss")]
    caps = capacity_descs(descs)
    # the shared path before any of the new tables: site 3's descriptors for everyone
    shared_descs = [dict(d) for d in descs[3]]
    yobs3 = np.tile(np.concatenate([d["yobs"] for d in descs[3]]), (S, 1))
    engine.set_targets(shared_descs)
    engine.set_sites(yobs3)
    shared = engine.evaluate_sites(*mods[:4], noise, site, rho=mods[4], want_ymod=True)
    batch0 = engine.evaluate_batch(*mods[:4], noise, rho=mods[4], want_ymod=True)

    engine.set_targets(caps)
    assert L.bh_sites_set_rf_axis(h, S, *axis()) == E.BH_EINVAL and "site table" in last_error(engine)
    # every existing sibling keeps refusing a receiver-function count that is not the descriptor's
    for entry in (L.bh_sites_set_x, L.bh_sites_set_x_all, L.bh_sites_set_missing, L.bh_sites_set_missing_gauss):
        assert entry(h, S, P(T["n"]), P(T["x"]), P(T["yobs"]), None) == E.BH_EINVAL
        assert "differs from its descriptor's" in last_error(engine)
    over = T["n"].copy()
    over[1, 1] = caps[1]["n"] + 1
    assert L.bh_sites_set_axes(h, S, P(over), P(T["x"]), P(T["yobs"]), None) == E.BH_EINVAL and "capacity" in last_error(engine)
    over[1, 1] = -1
    assert L.bh_sites_set_axes(h, S, P(over), P(T["x"]), P(T["yobs"]), None) == E.BH_EINVAL
    engine.set_sites_axes(T["n"], T["x"], T["yobs"])
    assert L.bh_sites_set_rf_axis(h, S, *axis()) == E.BH_EINVAL and "bh_sites_set_rf" in last_error(engine)
    # counts that differ and no axis table: the call names the entry point that is missing
    engine.set_sites_rf(T["p"], T["nsv"])
    with pytest.raises(E.EngineError, match="bh_sites_set_rf_axis"):
        engine.evaluate_sites(*mods[:4], noise, site, rho=mods[4])
    assert L.bh_sites_set_rf_axis(h, S - 1, *axis()) == E.BH_EINVAL and "nsites" in last_error(engine)
    for k in range(4):
        a = axis()
        a[k] = None
        assert L.bh_sites_set_rf_axis(h, S, *a) == E.BH_EINVAL and "null" in last_error(engine)

    def refused(code, word, **kw):
        assert L.bh_sites_set_rf_axis(h, S, *axis(**kw)) == code, kw
        assert word in last_error(engine), last_error(engine)

    def put(key, value, dtype=None):
        a = T[key].copy()
        a[2, 1] = value
        return {key: a}

    for bad in (96, 2, 0, -128):
        refused(E.BH_EINVAL, "power of two", **put("nsamp", bad))
    refused(E.BH_EINVAL, "below the site's sample count", **put("nsamp", 32))        # site 2 has 65 samples
    refused(E.BH_EUNSUPPORTED, "16384", **put("nsamp", 32768))
    for bad in (0.0, -5.0, np.nan, np.inf):
        refused(E.BH_EINVAL, "fsamp and gauss", **put("fsamp", bad))
        refused(E.BH_EINVAL, "fsamp and gauss", **put("gauss", bad))
    for bad in (np.nan, -np.inf):
        refused(E.BH_EINVAL, "tshift", **put("tshift", bad))
    # the columns of other targets are unread
    junk = {k: T[k].copy() for k in ("nsamp", "fsamp", "tshift", "gauss")}
    junk["nsamp"][:, 0], junk["fsamp"][:, 0], junk["tshift"][:, 0], junk["gauss"][:, 0] = -7, np.nan, np.inf, -1.0
    engine.set_sites_rf_axis(junk["nsamp"], junk["fsamp"], junk["tshift"], junk["gauss"])
    own = engine.evaluate_sites(*mods[:4], noise, site, rho=mods[4], want_ymod=True)
    engine.set_sites_rf_axis(T["nsamp"], T["fsamp"], T["tshift"], T["gauss"])
    again = engine.evaluate_sites(*mods[:4], noise, site, rho=mods[4], want_ymod=True)
    for a, b in zip(own, again):
        assert np.array_equal(bits(a), bits(b))
    assert L.bh_sites_set_rf_axis(h, S, *axis(nsamp=np.full_like(T["nsamp"], 16384))) == E.BH_OK      # 16384 is served
    engine.set_sites_rf_axis(T["nsamp"], T["fsamp"], T["tshift"], T["gauss"])
    # 512 / 512 / 20 Hz / 5.0: every sample of the transform kept, jc = 255 < 256 -- against its own one-site call
    full = [[rf_desc(E.LAW_EXP, 0, AXES[4], 6.4, 0.0, rs)], [rf_desc(E.LAW_EXP, 0, AXES[1], 7.0, 0.0, rs)]]
    refs = one_site_calls(engine, full, mods, noise[:, :2])
    register(engine, full)
    two = (np.arange(B) % 2).astype(np.int32)
    assert_rule(engine.evaluate_sites(*mods[:4], noise[:, :2], two, rho=mods[4], want_ymod=True), refs, full, two, np.arange(B), "512 of 512")
    # bh_evaluate_batch never reads the tables
    register(engine, descs)
    engine.set_targets(shared_descs)
    for a, b in zip(engine.evaluate_batch(*mods[:4], noise, rho=mods[4], want_ymod=True), batch0):
        assert np.array_equal(bits(a), bits(b))
    # set_sites, set_sites_rf and set_targets drop the axis table
    for drop in ("sites_rf", "sites_axes", "targets"):
        register(engine, descs)
        if drop == "sites_rf":
            engine.set_sites_rf(T["p"], T["nsv"])
        elif drop == "sites_axes":
            engine.set_sites_axes(T["n"], T["x"], T["yobs"])
            engine.set_sites_rf(T["p"], T["nsv"])
        else:
            engine.set_targets(caps)
            engine.set_sites_axes(T["n"], T["x"], T["yobs"])
            engine.set_sites_rf(T["p"], T["nsv"])
        with pytest.raises(E.EngineError, match="bh_sites_set_rf_axis"):
            engine.evaluate_sites(*mods[:4], noise, site, rho=mods[4])
    # ... and the shared path's bits are what they were before the tables were registered and dropped
    register(engine, descs)
    engine.set_targets(shared_descs)
    engine.set_sites(yobs3)
    for a, b in zip(engine.evaluate_sites(*mods[:4], noise, site, rho=mods[4], want_ymod=True), shared):
        assert np.array_equal(bits(a), bits(b))


def test_gauss_law_refusals(engine):
    """counts that differ under the Gauss law need the padded class table, and the in-kernel mat-vec does not serve them"""
    rs = np.random.RandomState(5)
    spec = [((128, 40, 5.0, 2.0, 1.0), 0.90), ((128, 64, 5.0, 0.0, 2.5), 0.94)]
    descs = gauss_sites(spec, rs)
    B = 16
    mods = models(rs, B, 10)
    noise = np.tile([0.0, 0.05, 0.0, 0.05], (B, 1))
    site = (np.arange(B) % 2).astype(np.int32)
    register(engine, descs)
    with pytest.raises(E.EngineError, match="bh_sites_set_gauss"):
        engine.evaluate_sites(*mods[:4], noise, site, rho=mods[4])
    before = engine.tuning("no_mfma")
    engine.set_tuning("no_mfma", 1)
    eng = None
    try:
        eng = E.Engine(0)
        register(eng, descs, {1: padded_classes(spec, 64)})
        with pytest.raises(E.EngineError, match="BH_NO_MFMA"):
            eng.evaluate_sites(*mods[:4], noise, site, rho=mods[4])
    finally:
        if eng is not None:
            eng.close()
        engine.set_tuning("no_mfma", before)


def test_the_axis_table_drops_the_laws_and_the_classes(engine):
    """bh_sites_set_rf_axis anew: the law table and the class tables registered on top of the axis table are gone -- the call is
    refused for the class table it needs again, and a class of -1 for a site that has the target is no longer accepted"""
    rs = np.random.RandomState(5)
    spec = [((128, 40, 5.0, 2.0, 1.0), 0.90), ((128, 64, 5.0, 0.0, 2.5), 0.94)]
    descs = gauss_sites(spec, rs)
    B = 16
    mods = models(rs, B, 10)
    noise = np.tile([0.0, 0.05, 0.0, 0.05], (B, 1))
    site = (np.arange(B) % 2).astype(np.int32)
    class_of, rinv, logdet = padded_classes(spec, 64)
    under_laws = np.array([class_of[0], -1], np.int32)            # site 1's trace under the nocorr law: no class
    T = register(engine, descs)
    engine.set_sites_laws(np.array([[E.LAW_NOCORR, E.LAW_GAUSS], [E.LAW_NOCORR, E.LAW_NOCORR]], np.int32))
    engine.set_sites_gauss(1, under_laws, rinv, logdet)
    assert (engine.evaluate_sites(*mods[:4], noise, site, rho=mods[4])[2] == 0).any()
    engine.set_sites_rf_axis(T["nsamp"], T["fsamp"], T["tshift"], T["gauss"])
    with pytest.raises(E.EngineError, match="bh_sites_set_gauss"):
        engine.evaluate_sites(*mods[:4], noise, site, rho=mods[4])
    with pytest.raises(E.EngineError, match="has the target"):
        engine.set_sites_gauss(1, under_laws, rinv, logdet)
    engine.set_sites_gauss(1, class_of, rinv, logdet)
    assert (engine.evaluate_sites(*mods[:4], noise, site, rho=mods[4])[2] == 0).any()


# ---- chains ------------------------------------------------------------------------------------------------
PRIORS = dict(vpvs=(1.4, 2.1), layers=(1, 10), vs=(2, 5), z=(0, 60), rfnoise_corr=(0.35, 0.75),
              rfnoise_sigma=(1e-5, 0.05), swdnoise_corr=0., swdnoise_sigma=(1e-5, 0.1))
# (samples, rate, shift, gauss): transforms of 128, 256 and 512 points
CHAIN_AXES = [(64, 5.0, 0.0, 1.0), (100, 10.0, 2.0, 2.5), (201, 5.0, 5.0, 2.5)]
CHAIN_AXES_64 = [(40, 5.0, 0.0, 1.0), (60, 10.0, 2.0, 2.5), (64, 5.0, 5.0, 2.5)]
CHAIN_P = (5.5, 6.4, 7.5)
CHAIN_CORR = (0.94, 0.98, 0.98)


def chain_site(s, axes, have_rf=True, as_slots=False):
    rs = np.random.RandomState(300 + s)
    per = np.linspace(3.0, 40.0, 12)
    t1 = bh.RayleighDispersionPhase(per, 3.2 + 0.015 * per + rs.normal(0, 0.02, per.size))
    n, fsamp, tshift, gauss = axes[s]
    x = np.arange(n) / fsamp - tshift
    t2 = bh.PReceiverFunction(x, 0.4 * np.exp(-(x / 0.6) ** 2) + 0.1 * np.exp(-((x - 4.0) / 0.8) ** 2) + rs.normal(0, 0.01, n))
    t2.moddata.plugin.set_modelparams(gauss=gauss, p=CHAIN_P[s])
    row = [t1, t2 if have_rf else None]
    return row if as_slots else bh.JointTarget([t for t in row if t is not None])


class _RefUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if module.startswith("BayHunter"):
            return type(name, (object,), {})
        return super().find_class(module, name)


def walk_and_compare(st, one_site, priors, depth, tmp_path, save, C=3):
    """DeviceChains over the sites against the one-site runs: samples of both phases, the proposal counters and (save) the saved
    folders, bit for bit.  priors: one dict, or one per site"""
    S = st.nsites
    init = dict(nchains=1, iter_burnin=100, iter_main=50, acceptance=(40, 80), thickmin=0.1, lvz=0.1, hvz=None, rcond=1e-5,
                maxmodels=15, savepath=str(tmp_path / "multi"))
    dc = DeviceChains(st, C, init, priors, seed=77, spec_depth=depth).run()
    paths = dc.save() if save else None
    state = dc.state_host()
    for s in range(S):
        ip = dict(init, savepath=str(tmp_path / "one" / st.names[s]), station=st.names[s])
        pr = priors[s] if isinstance(priors, (list, tuple)) else priors
        one = DeviceChains(one_site(s), C, ip, pr, seed=77, chain_offset=s * C, spec_depth=depth).run()
        for phase in ("p1", "p2"):
            a, b = dc.samples(phase, site=s), one.samples(phase)
            assert set(a) == set(b)
            for k in a:
                assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=True), "site %d %s: %s" % (s, phase, k)
        assert np.all(a["likes"] > -1e14), "site %d: a chain sits on a failed model" % s     # (the walks are real ones)
        own = one.state_host()
        for k in ("proposed", "accepted"):
            if k in own and own[k] is not None:
                assert np.array_equal(state[k][..., s * C:(s + 1) * C], own[k]), "site %d: %s" % (s, k)
        if paths is not None:       # the saved folder of a site is that of its one-site run
            dpath = one.save()
            files = sorted(f for f in os.listdir(dpath) if f.endswith(".npy"))
            assert files and files == sorted(f for f in os.listdir(paths[s]) if f.endswith(".npy"))
            for f in files:
                assert np.array_equal(np.load(os.path.join(dpath, f)), np.load(os.path.join(paths[s], f)), equal_nan=True), f
            with open(os.path.join(paths[s], "%s_config.pkl" % st.names[s]), "rb") as f:
                cfg = _RefUnpickler(f).load()
            pl, want = cfg["targets"][-1].moddata.plugin, one_site(s).targets[-1].moddata.plugin
            assert (pl.nsamp, pl.fsamp, pl.tshft, pl.modelparams["gauss"], pl.modelparams["p"]) == \
                   (want.nsamp, want.fsamp, want.tshft, want.modelparams["gauss"], want.modelparams["p"])
            assert np.array_equal(cfg["targets"][-1].obsdata.x, one_site(s).targets[-1].obsdata.x)
    return dc


@pytest.mark.parametrize("depth", [None, 1, 3])
def test_chains_walk_the_one_site_trajectories(depth, tmp_path):
    """3 sites x 3 chains (a site boundary inside a window's wavefront), a Rayleigh phase curve beside a P receiver function on
    the site's own axis with its own filter and ray parameter, exponential law: samples of both phases, counters and the saved
    folders are the one-site runs'"""
    st = bh.SiteTargets([chain_site(s, CHAIN_AXES) for s in range(3)], names=["st%d" % s for s in range(3)],
                        per_site_x="all", per_site_rf="all")
    walk_and_compare(st, lambda s: chain_site(s, CHAIN_AXES), PRIORS, depth, tmp_path, save=depth is None)


def test_chains_under_the_gauss_law(tmp_path):
    """rfnoise_corr fixed at 0.94 / 0.98 / 0.98 (the Gauss law), n = 40 / 60 / 64 in columns of 64: the padded classes give the
    one-site bits (test_gauss_law_capacity_64)"""
    priors = [dict(PRIORS, rfnoise_corr=c) for c in CHAIN_CORR]
    st = bh.SiteTargets([chain_site(s, CHAIN_AXES_64) for s in range(3)], names=["st%d" % s for s in range(3)],
                        per_site_x="all", per_site_rf="all", per_site_corr=True)
    walk_and_compare(st, lambda s: chain_site(s, CHAIN_AXES_64), priors, 1, tmp_path, save=False)


def test_chains_with_a_site_that_lacks_the_trace(tmp_path):
    st = bh.SiteTargets([chain_site(s, CHAIN_AXES, have_rf=s != 1, as_slots=True) for s in range(3)], names=["st%d" % s for s in range(3)],
                        per_site_x="all", per_site_rf="all", missing=True)
    walk_and_compare(st, lambda s: chain_site(s, CHAIN_AXES, have_rf=s != 1), PRIORS, 1, tmp_path, save=False)
