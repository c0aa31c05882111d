"""Posterior residuals of many sites on the GPU (include/bh_engine_posterior_resid.h, bayhunter_amd/datafits.py:
posterior_residuals) against the restatement tests/resid_ref.py, which tests/test_resid_ref.py holds to exact rational arithmetic.
The kernel is fed hand-made synthetics first -- every column of every row bit for bit, NaN included -- and then runs behind the
forward models, where the expected synthetics are those of SiteTargets.evaluate_batch on the restated layers (as in
tests/test_gpu_posterior_datafits.py) and every statistic is the one posterior_scalars gives for the restated columns."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import REPO
import bayhunter_amd as bh
from bayhunter_amd import engine as E
from bayhunter_amd import datafits as DF
from bayhunter_amd.posterior import _ptr
import datafit_ref as DR
import resid_ref as RR

pytestmark = pytest.mark.gpu
QS = DF.DEFAULT_QUANTILES
STAT_KEYS = ("count", "nan", "min", "max", "median", "mean", "std", "quantiles")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def same_bits(a, b, what=()):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, what
    bad = np.argwhere(bits(a) != bits(b))
    assert not len(bad), (what, bad[:5].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])


def same(a, b, what=()):
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), what
        for k in a:
            same(a[k], b[k], what + (k,))
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, what + (i,))
    elif a is None or b is None or isinstance(a, str):
        assert a == b, what
    else:
        x, y = np.asarray(a), np.asarray(b)
        assert x.dtype == y.dtype and x.shape == y.shape, what
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), what


# ---- 1. the header ----------------------------------------------------------------------------------------------------------

def test_the_constants_and_symbols_mirror_the_header():
    txt = open(REPO + "/include/bh_engine_posterior_resid.h").read()
    defs = {k: int(v) for k, v in re.findall(r"^#define\s+(BH_[A-Z0-9_]+)\s+(-?\d+)\b", txt, flags=re.M)}
    assert defs == dict(BH_SCALARS_RESID=E.SCALARS_RESID, BH_RESID_MAXLAG=E.RESID_MAXLAG, BH_RESID_FIXED=E.RESID_FIXED)
    assert (E.SCALARS_RESID, E.RESID_MAXLAG, E.RESID_FIXED) == (5, RR.MAXLAG, RR.FIXED) and DF.RESID_NAMES == RR.NAMES
    body = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert sorted(set(re.findall(r"\b(bh_[a-z_0-9]+)\s*\(", body))) == sorted(E.POSTERIOR_RESID_SYMBOLS)
    lib = C.CDLL(E.LIB_PATH)
    assert all(hasattr(lib, n) for n in E.POSTERIOR_RESID_SYMBOLS) and lib.bh_abi_version() == 10


# ---- 2. the kernel alone ----------------------------------------------------------------------------------------------------

NCOL = np.array([[1, 5], [64, 0], [65, 130]], np.int32)   # n <= l, the 64 / 65 strand edge, more than two rounds, a missing slot
ROWS = (1, 64, 70)


def hand_case(ncol=NCOL, rows=ROWS, seed=11, special=True):
    """synthetics, flags and noise by input row, the sites' rows interleaved"""
    rs = np.random.RandomState(seed)
    S, nt = ncol.shape
    ldy = int(ncol.max(axis=0).sum())
    site = rs.permutation(np.concatenate([np.full(n, s, np.int32) for s, n in enumerate(rows)]))
    N = len(site)
    yobs = rs.normal(0.0, 1.0, (S, ldy))
    ymod = yobs[site] + rs.normal(0.0, 0.05, (N, ldy)) * 10.0 ** rs.randint(-2, 3, (N, 1))
    err = np.zeros(N, np.int32)
    noise = np.stack([rs.uniform(0.0, 0.99, N), rs.uniform(0.01, 0.1, N)] * nt, axis=1)
    if special:
        last = np.flatnonzero(site == S - 1)
        err[last[[3, 40]]] = (1, 7)                      # failed forward runs
        err[np.flatnonzero(site == 1)[63]] = 2
        ymod[last[5]] = yobs[S - 1]                      # a residual of zero
        noise[last[6], 1::2] = 0.0                       # sigma = 0
    g = 1.0 / np.sqrt(rs.uniform(1.0, 9.0, (S, ldy)))
    return dict(site=site, ncol=ncol, yobs=yobs, ymod=ymod, err=err, noise=noise, g=g, ldy=ldy)


def loaded_order(ld):
    """every loaded row's index in the input: the USER set of an index column, gathered row by row"""
    ld.attach(np.arange(ld.N, dtype=np.float64)[:, None], False)
    return ld.gather(E.SCALARS_USER, np.arange(ld.nrows), 1)[:, 0].astype(np.int64)


def run_fill(engine, c, L, batch, perm=None, dtype=np.float64, device=False, g=None):
    """the RESID set of the case, its input rows permuted, as values by (unpermuted) input row, and failed[S]"""
    import torch
    N, (S, nt) = len(c["site"]), c["ncol"].shape
    perm = np.arange(N) if perm is None else perm
    rows = np.tile(np.array([3.0, 4.0, 5.0, 30.0], np.float32), (N, 1))
    ld = DF._DataLoaded(rows, c["site"][perm], engine, S)
    try:
        assert ld.nrows == N
        orig = loaded_order(ld)
        nz = np.ascontiguousarray(c["noise"][perm].astype(dtype))
        ntup = DF._noise_rows(torch.from_numpy(nz).cuda() if device else nz, N, nt)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        keep, failed = [], None
        for r0, r1 in DF.plan_batches(N, batch):
            idx = perm[orig[r0:r1]]
            ym, er = torch.from_numpy(c["ymod"][idx]).cuda(), torch.from_numpy(c["err"][idx]).cuda()
            keep.append((ym, er))                        # (the call only enqueues its kernel)
            failed = ld.resid_fill(stream, r0, r1 - r0, c["ldy"], ym, er, c["ncol"], L, c["yobs"], g, ntup)
        Q = nt * (E.RESID_FIXED + L)
        q = np.zeros(1, np.int32)
        engine._check(engine._L.bh_posterior_scalar_cols(ld._p, E.SCALARS_RESID, _ptr(q)))
        assert q[0] == Q
        vals = ld.gather(E.SCALARS_RESID, np.arange(N), Q)
    finally:
        ld.close()
    out = np.empty((N, Q))
    out[perm[orig]] = vals
    return out, failed


_REF = {}


def hand_ref(c, L, dtype, g):
    key = (L, np.dtype(dtype).str, g is not None)
    if key not in _REF:
        _REF[key] = RR.resid_set(c["ymod"], c["err"], c["site"], c["ncol"], c["yobs"], c["noise"].astype(dtype), L, g)
    return _REF[key]


HAND = hand_case()


@pytest.mark.parametrize("batch,dtype,device,permute,weights", [
    (135, np.float64, False, 0, False), (7, np.float32, True, 1, False), (64, np.float64, True, 2, True),
    (135, np.float32, False, 0, True), (7, np.float64, False, 3, False)])
def test_every_column_of_every_row(batch, dtype, device, permute, weights, engine):
    c, L = HAND, 8
    g = c["g"] if weights else None
    want = hand_ref(c, L, dtype, g)
    perm = np.random.RandomState(permute).permutation(len(want)) if permute else None
    got, failed = run_fill(engine, c, L, batch, perm, dtype, device, g)
    same_bits(got, want, (batch, device, permute, weights))
    assert failed.tolist() == [0, 1, 2]
    again, _ = run_fill(engine, c, L, batch, perm, dtype, device, g)
    same_bits(again, got)
    # what the case is there to cover
    last = np.flatnonzero(c["site"] == 2)
    W = E.RESID_FIXED + L
    assert np.isnan(want[c["err"] != 0]).all() and np.isnan(want[c["site"] == 1][:, W:]).all()
    z = want[last[5]]
    assert z[0] == 0.0 and z[1] == 0.0 and z[2] == 0.0 and np.isnan(z[4:W]).all() and not np.isnan(z[3])
    s0 = want[last[6]]
    assert np.isnan(s0[2]) and np.isnan(s0[W + 2]) and not np.isnan(s0[[0, 1, 3, 4, 5]]).any()
    first = want[np.flatnonzero(c["site"] == 0)[0]]
    assert np.isnan(first[4:W]).all() and not np.isnan(first[:4]).any()          # n = 1: no lag at all
    assert not np.isnan(first[W:W + 5 + 4]).any() and np.isnan(first[W + 5 + 4:]).all()   # n = 5: the lags 1 .. 4
    assert np.isfinite(got[~np.isnan(got)]).all()


@pytest.mark.parametrize("L", (1, E.RESID_MAXLAG))
def test_the_least_and_the_largest_lag_count(L, engine):
    c = hand_case(np.array([[33]], np.int32), (5,), seed=3, special=False)
    got, failed = run_fill(engine, c, L, 5)
    same_bits(got, RR.resid_set(c["ymod"], c["err"], c["site"], c["ncol"], c["yobs"], c["noise"], L))
    assert got.shape == (5, 5 + L) and not np.isnan(got).any() and failed.tolist() == [0]


# ---- 3. a site alone --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", (1, 2))
def test_a_site_alone_has_the_bits_it_has_among_the_others(s, engine):
    c, L = HAND, 8
    every, _ = run_fill(engine, c, L, 64, g=c["g"])
    mine = c["site"] == s
    ldy = int(c["ncol"][s].sum()) if s == 1 else c["ldy"]                   # (site 1 alone: its 64 columns are the whole block)
    one = dict(site=np.zeros(int(mine.sum()), np.int32), ncol=c["ncol"][s:s + 1], yobs=np.ascontiguousarray(c["yobs"][s:s + 1, :ldy]),
               ymod=np.ascontiguousarray(c["ymod"][mine][:, :ldy]), err=c["err"][mine], noise=c["noise"][mine], ldy=ldy)
    alone, _ = run_fill(engine, one, L, 64, g=np.ascontiguousarray(c["g"][s:s + 1, :ldy]))
    same_bits(alone, every[mine], (s,))


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing_and_leave_the_set_unformed(engine):
    import torch
    c, L = HAND, 8
    N, nt, ldy = len(c["site"]), 2, c["ldy"]
    Lb = engine._L
    rows = np.tile(np.array([3.0, 4.0, 5.0, 30.0], np.float32), (N, 1))
    ym, er = torch.from_numpy(c["ymod"][:64].copy()).cuda(), torch.zeros(64, dtype=torch.int32).cuda()
    yp, ep = C.c_void_p(ym.data_ptr()), C.c_void_p(er.data_ptr())
    noise = np.ascontiguousarray(c["noise"])
    ld = DF._DataLoaded(rows, c["site"], engine, 3)

    def call(r0=0, nb=64, ldy=ldy, ncol=c["ncol"], L=L, yobs=c["yobs"], g=None, nld=2 * nt, elem=8):
        return Lb.bh_posterior_resid_fill(ld._p, None, r0, nb, ldy, yp, ep, nt, _ptr(np.ascontiguousarray(ncol, np.int32)), L,
                                          _ptr(None if yobs is None else np.ascontiguousarray(yobs)), _ptr(g), E.HOST, elem, nld,
                                          _ptr(noise), None)

    def refused(rc, text):
        assert rc == E.BH_EINVAL
        with pytest.raises(E.EngineError, match=text):
            engine._check(rc)
        with pytest.raises(E.EngineError, match="RESID set does not exist yet"):
            engine._check(Lb.bh_posterior_scalar_cols(ld._p, E.SCALARS_RESID, _ptr(np.zeros(1, np.int32))))

    try:
        refused(call(L=0), "BH_RESID_MAXLAG")
        refused(call(L=E.RESID_MAXLAG + 1), "BH_RESID_MAXLAG")
        refused(call(nld=2 * nt - 1), "noise_ld")
        refused(call(elem=2), "float32 or float64")
        refused(call(ldy=E.DATAFIT_MAXCOLS + 1), "BH_DATAFIT_MAXCOLS")
        refused(call(ldy=ldy + 1), "add up")
        refused(call(yobs=None), "null")
        refused(call(r0=64), "in order")
        for other in (dict(ncol=np.array([[1, 5], [63, 0], [65, 130]])), dict(yobs=c["yobs"] + 1.0), dict(L=L - 1), dict(g=c["g"]),
                      dict(nld=2 * nt + 1), dict(r0=65, nb=1)):
            engine._check(call())                           # a fill under way, rows [0, 64) done
            refused(call(**dict(dict(r0=64, nb=64), **other)), "differs|in order")
            refused(call(r0=64), "in order")                # (the refusal ended the fill)
        # the same handle still fills
        engine._check(call())
        engine._check(call(r0=64))
        engine._check(call(r0=128, nb=N - 128))
        q = np.zeros(1, np.int32)
        engine._check(Lb.bh_posterior_scalar_cols(ld._p, E.SCALARS_RESID, _ptr(q)))
        assert q[0] == nt * (E.RESID_FIXED + L)
        refused(call(L=0), "BH_RESID_MAXLAG")                # ... and a refusal unforms the set again
    finally:
        ld.close()


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------

ML = 6
PERIODS = np.array([4.0, 8.0, 14.0, 22.0, 33.0])
T_RF = np.arange(48) * 0.5 - 5.0


def tiny_sites():
    """two sites: Rayleigh phase velocities at 5 periods under nocorr_scalederr (the weights g) and a P receiver function of 48
    samples under the exponential law"""
    rs = np.random.RandomState(8)
    sites = []
    for s in range(2):
        t1 = bh.RayleighDispersionPhase(PERIODS, 3.3 + 0.02 * PERIODS + rs.normal(0, 0.02, 5), yerr=rs.uniform(0.01, 0.04, 5))
        t1.set_noise_law("nocorr_scalederr")
        t2 = bh.PReceiverFunction(T_RF, rs.normal(0, 0.05, T_RF.size))
        t2.moddata.plugin.set_modelparams(gauss=1.0, p=6.4)
        t2.set_noise_law("exp")
        sites.append(bh.JointTarget([t1, t2]))
    return bh.SiteTargets(sites)


def prior_rows(rs, n):
    rows = np.full((n, 2 * ML), np.nan)
    for i in range(n):
        k = rs.randint(2, ML + 1)
        rows[i, :k] = np.sort(rs.uniform(2.2, 4.7, k)) + rs.uniform(-0.3, 0.3, k)
        rows[i, k:2 * k] = np.sort(rs.uniform(0, 60, k))
    return rows.astype(np.float32), rs.uniform(1.6, 1.9, n).astype(np.float32)


def test_residuals_of_two_tiny_sites(engine):
    rs = np.random.RandomState(2027)
    N, L = 83, 10
    rows, vpvs = prior_rows(rs, N)
    site = rs.permutation((np.arange(N) % 2).astype(np.int32))
    rows[int(np.flatnonzero(site == 1)[4]), 0] = 150.0                       # fails without a search
    noise = np.stack([rs.uniform(0, 0.5, N), rs.uniform(0.01, 0.1, N), rs.uniform(0.5, 0.99, N), rs.uniform(0.01, 0.1, N)],
                     axis=1).astype(np.float32)
    st = tiny_sites()
    got = bh.posterior_residuals(st, rows, vpvs, noise, site=site, maxlag=L, engine=engine)
    # the expected synthetics, as tests/test_gpu_posterior_datafits.py obtains them
    nlay, h, vp, vs, rho = DR.layer_batch(rows, vpvs, None)
    _, _, err, ymod = st.evaluate_batch(nlay, h, vp, vs, np.tile([0.0, 1.0], (N, 2)), site, rho=rho, want_ymod=True)
    assert int((err != 0).sum()) == 1
    ncol = st._counts()
    yobs, g, laws = DF._resid_tables(st)
    assert g is not None and (g[:, :5] <= 1.0).all() and (g[:, :5].max(axis=1) == 1.0).all() and (g[:, 5:] == 1.0).all()
    for s in range(2):
        ye = np.asarray(st.site(s).targets[0].obsdata.yerr)
        same_bits(g[s, :5], 1.0 / np.sqrt(ye / ye.min()))
    want = RR.resid_set(ymod, err, site, ncol, yobs, noise, L, g)
    W = E.RESID_FIXED + L
    ref = bh.posterior_scalars(rows, dict(c=want), site=site, nlayers=False, engine=engine, nsites=2, quantiles=QS)
    assert len(got) == 2
    for s in range(2):
        mine = site == s
        assert got[s]["rows"] == int(mine.sum()) and got[s]["failed"] == int((err[mine] != 0).sum()) == s
        assert sorted(got[s]) == ["failed", "prf", "rdispph", "rows"]
        for t, name in enumerate(("rdispph", "prf")):
            d = got[s][name]
            assert d["n"] == ncol[s, t] and d["law"] == ("nocorr_scalederr", "exp")[t] and d["lags"].tolist() == list(range(1, L + 1))
            assert d["acf_white95"] == 1.96 / np.sqrt(ncol[s, t])
            for k, col in enumerate(RR.NAMES):
                w = ref[s]["c"][t * W + k]
                for key in STAT_KEYS:
                    same_bits(d[col][key], w[key], (s, name, col, key))
                assert d[col]["count"] == got[s]["rows"] - got[s]["failed"]
            for l in range(L):
                w = ref[s]["c"][t * W + E.RESID_FIXED + l]
                for key in STAT_KEYS[:-1]:
                    same_bits(d["acf"][key][l], w[key], (s, name, "acf", l, key))
                same_bits(d["acf"]["quantiles"][:, l], w["quantiles"], (s, name, "acf", l))
            assert d["acf"]["quantiles"].shape == (len(QS), L)
            same_bits(d["acf_model"], RR.acf_model(d["law"], d["corr"]["median"], L))
            assert (d["acf"]["count"][:min(L, ncol[s, t] - 1)] > 0).all() and (d["acf"]["count"][ncol[s, t] - 1:] == 0).all()
        assert not got[s]["rdispph"]["acf_model"].any() and got[s]["prf"]["acf_model"][0] == got[s]["prf"]["corr"]["median"]
    # from device tensors, in forward batches of 16 rows, one site per group: the same bits
    import torch
    t = lambda a: torch.from_numpy(a).cuda()
    same(DF._datafits(st, t(rows), t(vpvs), site=t(site), engine=engine, batch=16, max_bytes=1, data=False,
                      residuals=dict(noise=t(noise), maxlag=L)), got)
    # ... and beside the data fits, which stay what they were
    plain = bh.posterior_datafits(st, rows, vpvs, site=site, engine=engine)
    both = bh.posterior_datafits(st, rows, vpvs, site=site, engine=engine, residuals=dict(noise=noise, maxlag=L))
    for s in range(2):
        for name in ("rdispph", "prf"):
            same(both[s][name].pop("residuals"), got[s][name], (s, name))
    same(both, plain)
    with pytest.raises(ValueError):
        bh.posterior_residuals(st, rows, vpvs, noise, site=site, maxlag=33, engine=engine)
    with pytest.raises(ValueError):
        bh.posterior_residuals(st, rows, vpvs, noise[:, :3], site=site, engine=engine)


# ---- 6. the chains' record ----------------------------------------------------------------------------------------------------

def test_chains_read_their_device_record(tmp_path, engine):
    """2 sites x 2 chains: the residuals from the device store, its noise table included, equal those of the function on the host
    arrays of samples(); exclude_chains drops rows; the saved folders agree"""
    from bayhunter_amd.device_chains import DeviceChains
    from test_gpu_posterior_datafits import chain_targets
    from test_gpu_sites_priors import SITE_INIT, SITE_PRIORS
    inits = [dict(SITE_INIT[s], iter_burnin=150, iter_main=150, maxmodels=150, savepath=str(tmp_path)) for s in range(2)]
    pri = [SITE_PRIORS[0], SITE_PRIORS[2]]
    dc = DeviceChains(chain_targets(), 2, inits, pri, seed=5, search="fast", record="device").run()
    a = dc.posterior_residuals(maxlag=6)
    T = dc.nsamples("p2")
    assert len(a) == 2 and all(x["rows"] == 2 * T for x in a)
    h = dc.samples("p2")
    n, Cn = h["models"].shape[:2]
    site = np.tile(np.repeat(np.arange(2, dtype=np.int32), 2), n)
    b = bh.posterior_residuals(dc.sites, h["models"].reshape(n * Cn, -1), h["vpvs"].reshape(-1), h["noise"].reshape(n * Cn, -1),
                               site=site, maxlag=6, mantle=[p.get("mantle") for p in pri], engine=engine)
    same(a, b)
    refs = [k for k in a[0] if k not in ("rows", "failed")]
    assert refs and all(a[0][k]["rms"]["count"] == 2 * T - a[0]["failed"] for k in refs)
    x = dc.posterior_residuals(maxlag=6, exclude_chains=(1,))
    assert x[0]["rows"] == T and x[1]["rows"] == 2 * T
    same(x[1], a[1])
    paths = dc.save(str(tmp_path))
    for p in paths:
        bh.save_final_distribution(p, maxmodels=300, dev=10.0)
    laws = {t.ref: t.law() for t in dc.sites.targets if t.law() != "gauss"}
    f = bh.residuals_from_storage(paths, maxlag=6, laws=laws, engine=engine)
    for s in range(2):
        assert f[s]["rows"] == a[s]["rows"]
        for t in dc.sites.site(s).targets:
            # (the files hold float64 copies of the float32 rows: vp = vs * vpvs is then a float64 product and the synthetics agree
            # to 1e-5 of their peak, not bit for bit -- tests/test_gpu_posterior_datafits.py; an rms moves by no more than its
            # synthetics do, and the observed data's peak is within a factor 2 of theirs)
            k = t.ref
            assert f[s][k]["n"] == a[s][k]["n"]
            same_bits(f[s][k]["corr"]["median"], a[s][k]["corr"]["median"])
            assert abs(f[s][k]["rms"]["median"] - a[s][k]["rms"]["median"]) <= 2e-5 * np.max(np.abs(t.obsdata.y))


def test_tempered_chains_take_their_cold_rows(engine):
    """one ladder of 4 temperatures per site: the beta = 1 rows are selected on the device"""
    from bayhunter_amd.device_chains import DeviceChains
    from test_gpu_chains import SETUPS
    from test_gpu_posterior_scalars import site_targets
    su = SETUPS["exp"]
    T = 80
    init = dict(su["init"], iter_burnin=160, iter_main=T, maxmodels=T)
    ladder = np.repeat(np.arange(2), 4)
    betas = np.tile(1.0 / np.geomspace(1.0, 20.0, 4), 2)
    dc = DeviceChains(site_targets(), 4, init, su["priors"], seed=6, betas=betas, ladder=ladder, swap_every=20, record="device").run()
    cold = dc.posterior_residuals(maxlag=4)                                   # cold_only by default
    every = dc.posterior_residuals(maxlag=4, cold_only=False)
    mantle = [p.get("mantle") for p in dc.site_priors]
    for s in range(2):
        h = dc.samples("p2", cold_only=True, site=s)
        assert cold[s]["rows"] == T and every[s]["rows"] == 4 * T
        one = bh.posterior_residuals(bh.SiteTargets([dc.sites.site(s)]), h["models"].reshape(T, -1), h["vpvs"].reshape(T),
                                     h["noise"].reshape(T, -1), site=np.zeros(T, np.int32), maxlag=4, mantle=[mantle[s]], engine=engine)
        same(cold[s], one[0], (s, "cold"))
