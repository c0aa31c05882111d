"""Posterior data fits of many sites on the GPU (bayhunter_amd/datafits.py, include/bh_engine_posterior_datafit.h) against the
restatement tests/datafit_ref.py, which tests/test_datafit_ref.py holds to the reference's own outputs.  Under conftest's
reference search and exact arithmetic the forward results are the reference's bits, so the expected synthetics are those of
SiteTargets.evaluate_batch(..., want_ymod=True) on the restated layers, and everything but mean and std (1e-13 of the exact
rationals, the bound of test_gpu_posterior_scalars.py for the same sums) is compared bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import golden
import bayhunter_amd as bh
from bayhunter_amd import engine as E
from bayhunter_amd import datafits as DF
from bayhunter_amd.posterior import _keys_to_values, _ptr
import datafit_ref as DR

pytestmark = pytest.mark.gpu
KEYS = ("f32", "f64of32", "f64")
QS = DF.DEFAULT_QUANTILES
COUNTS = (0, 1, 2, 63, 64, 65, 257, 8193)          # rows per site; the last crosses the 8192-row chunk of the column passes
ML = 6
T_RF = np.arange(64) * 0.5 - 5.0                   # 64 samples at 2 Hz
PERIODS = np.array([4.0, 8.0, 14.0, 22.0, 33.0])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.dtype.str, a.shape, a.tobytes()


def same(a, b, what=()):
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), what
        for k in a:
            same(a[k], b[k], what + (k,))
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, what + (i,))
    elif a is None or b is None:
        assert a is None and b is None, what
    else:
        x, y = np.asarray(a), np.asarray(b)
        assert x.dtype == y.dtype and x.shape == y.shape, what
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), what


# ---- layers ---------------------------------------------------------------------------------------------------------------

def loaded_order(ld):
    """every loaded row's index in the input: the USER set of an index column, gathered row by row"""
    ld.attach(np.arange(ld.N, dtype=np.float64)[:, None], False)
    return ld.gather(E.SCALARS_USER, np.arange(ld.nrows), 1)[:, 0].astype(np.int64)


@pytest.mark.parametrize("key", KEYS)
def test_layers_are_the_references(key, engine):
    """the golden rows through bh_posterior_layers; site 0 without a mantle rule and site 1 with one in the same call"""
    import torch
    G = golden("datafit_golden.npz")
    rows, vpvs = G[key + "_rows"], G[key + "_vpvs"]
    N = len(rows)
    site = (np.arange(N) % 2).astype(np.int32)
    mantle = G["mantle"]
    ld = DF._DataLoaded(rows, site, engine, 2)
    try:
        assert ld.nrows == N
        fw = DF._Forward(engine, torch.device("cuda", 0), 64, rows.shape[1] // 2, 1, 1)   # (its buffers; batches of 64 rows)
        vt = DF._per_row(torch.from_numpy(vpvs).cuda(), N, "vpvs")
        got = {k: np.zeros((N, 21)) for k in ("h", "vp", "vs", "rho")}
        nlay, gsite = np.zeros(N, np.int32), np.zeros(N, np.int32)
        for r0, r1 in DF.plan_batches(N, 64):
            ld.layers(r0, r1, vt, np.array([-1.0, mantle[0]]), np.array([0.0, mantle[1]]), fw.buf, 64)
            torch.cuda.synchronize()
            for k in got:
                got[k][r0:r1] = fw.buf[k].cpu().numpy()[:, :r1 - r0].T
            nlay[r0:r1], gsite[r0:r1] = fw.buf["nlay"].cpu().numpy()[:r1 - r0], fw.buf["site"].cpu().numpy()[:r1 - r0]
        orig = loaded_order(ld)
        # a host vpvs gives the same layers
        nb = min(N, 64)
        ld.layers(0, nb, DF._per_row(vpvs, N, "vpvs"), np.array([-1.0, mantle[0]]), np.array([0.0, mantle[1]]), fw.buf, 64)
        torch.cuda.synchronize()
        assert np.array_equal(fw.buf["vp"].cpu().numpy()[:, :nb].T, got["vp"][:nb])
    finally:
        ld.close()
    assert sorted(orig) == list(range(N)) and np.array_equal(gsite, site[orig]) and list(gsite) == sorted(gsite)
    for tag, s in (("plain", 0), ("mantle", 1)):
        sel = gsite == s
        assert np.array_equal(nlay[sel], G["%s_%s_nlay" % (key, tag)][orig[sel]])
        for k in got:
            want = G["%s_%s_%s" % (key, tag, k)][orig[sel]].astype(np.float64)
            assert bits(got[k][sel]) == bits(want), (key, tag, k)


# ---- best -----------------------------------------------------------------------------------------------------------------

def test_best_of_every_site_and_chain(engine):
    import torch
    rs = np.random.RandomState(31)
    S, NCH, N = 4, 3, 900
    rows = np.full((N, 2 * ML), np.nan, np.float32)
    rows[:, 0:2], rows[:, 2:4] = (3.0, 4.0), (5.0, 30.0)                 # two layers: vs, vs, z, z
    site = rs.randint(0, 3, N).astype(np.int32)                          # site 3 has no row
    chain = rs.randint(0, NCH, N).astype(np.int32)
    chain[(site == 1) & (chain == 2)] = 0                                # (site 1, chain 2) has no row
    mis = np.round(rs.uniform(0.2, 0.9, N), 2)                           # two decimals: repeated least misfits inside a chain
    for s in range(3):
        for c in range(NCH):
            idx = np.flatnonzero((site == s) & (chain == c))
            if idx.size > 3:
                mis[idx[rs.randint(0, idx.size, 3)]] = mis[idx].min()
    out = rs.choice(N, 40, replace=False)
    site[out] = -1                                                       # dropped rows hold the least misfit of all
    mis[out] = 0.01
    want = DR.best_of_chains(site, chain, mis, S, NCH)
    assert (want[3] == -1).all() and want[1, 2] == -1 and (want[:3, :2] >= 0).all()

    def run(perm, mis_arg):
        ld = DF._DataLoaded(torch.from_numpy(rows[perm]).cuda(), torch.from_numpy(site[perm]).cuda(), engine, S)
        try:
            assert ld.dropped == 40
            b, pos = ld.best(NCH, *mis_arg(chain[perm], mis[perm]))
            order = loaded_order(ld)
        finally:
            ld.close()
        assert np.array_equal(pos >= 0, b >= 0) and np.array_equal(order[pos[pos >= 0]], b[b >= 0])
        return np.where(b >= 0, perm[np.maximum(b, 0)], -1)

    ident = np.arange(N)
    f32dev = lambda c, m: (torch.from_numpy(c).cuda(), torch.from_numpy(m.astype(np.float32)).cuda())   # float32 from the device
    f64host = lambda c, m: (c.copy(), m.copy())                                                          # float64 from the host
    a = run(ident, f64host)
    assert np.array_equal(a, want)
    assert np.array_equal(run(ident, f64host), a)                       # on a repeat
    w32 = DR.best_of_chains(site, chain, mis.astype(np.float32), S, NCH)
    assert np.array_equal(run(ident, f32dev), w32)
    for seed in (1, 2):
        perm = np.random.RandomState(seed).permutation(N)
        got = run(perm, f64host)                                        # the rows shuffled again: the same misfits win, and
        w = np.where(want >= 0, mis[np.maximum(want, 0)], np.nan)        # among equal ones the first in the new order
        g = np.where(got >= 0, mis[np.maximum(got, 0)], np.nan)
        assert np.array_equal(w, g, equal_nan=True)
        again = DR.best_of_chains(site[perm], chain[perm], mis[perm], S, NCH)
        assert np.array_equal(got, np.where(again >= 0, perm[np.maximum(again, 0)], -1))


# ---- fill and statistics --------------------------------------------------------------------------------------------------

def prior_rows(rs, n, dtype=np.float32):
    """prior-like rows of 2..ML layers and a vpvs each"""
    rows = np.full((n, 2 * ML), np.nan)
    for i in range(n):
        k = rs.randint(2, ML + 1)
        rows[i, :k] = np.sort(rs.uniform(2.2, 4.7, k)) + rs.uniform(-0.3, 0.3, k)
        rows[i, k:2 * k] = np.sort(rs.uniform(0, 60, k))
    return rows.astype(dtype), rs.uniform(1.6, 1.9, n).astype(dtype)


def site_targets(kind):
    """8 sites.  "plain": Rayleigh phase at 5 shared periods + P receiver function of 64 samples (ldy 69: it crosses a 64-column
    tile); "one": one period (ldy 1); "missing": per_site_x="all", missing=True -- site 1 lacks the receiver function, site 2
    has 3 of the 5 periods"""
    rs = np.random.RandomState(77)
    sites = []
    for s in range(len(COUNTS)):
        per = PERIODS[:1] if kind == "one" else PERIODS[:3] if (kind == "missing" and s == 2) else PERIODS
        t1 = bh.RayleighDispersionPhase(per, 3.3 + 0.02 * per + rs.normal(0, 0.02, per.size))
        t1.set_noise_law("nocorr")
        t2 = bh.PReceiverFunction(T_RF, rs.normal(0, 0.05, T_RF.size))
        t2.moddata.plugin.set_modelparams(gauss=1.0, p=6.4)
        t2.set_noise_law("nocorr")
        if kind == "one":
            sites.append([t1])
        elif kind == "missing":
            sites.append([t1, None if s == 1 else t2])
        else:
            sites.append([t1, t2])
    if kind == "missing":
        return bh.SiteTargets(sites, per_site_x="all", missing=True)
    return bh.SiteTargets([bh.JointTarget(t) for t in sites])


@pytest.fixture(scope="module")
def posterior_rows():
    """the rows of every site in shuffled order; two rows with a velocity above 100 km/s, which fail without a search"""
    rs = np.random.RandomState(2026)
    rows, vpvs = prior_rows(rs, sum(COUNTS))
    site = np.concatenate([np.full(n, s, np.int32) for s, n in enumerate(COUNTS)])
    bad = [int(np.flatnonzero(site == 5)[7]), int(np.flatnonzero(site == 7)[4000])]
    for i in bad:
        rows[i, 0] = 150.0
    perm = rs.permutation(len(rows))
    return dict(rows=rows[perm], vpvs=vpvs[perm], site=site[perm], bad=bad)


_EXPECTED = {}


def expected(kind, d, mantle=None):
    """the masked synthetics [N, ldy] of the restated layers through the host call, computed once per configuration"""
    if kind not in _EXPECTED:
        st = site_targets(kind)
        per_row = None if mantle is None else [mantle[s] for s in d["site"]]
        nlay, h, vp, vs, rho = DR.layer_batch(d["rows"], d["vpvs"], per_row)
        noise = np.tile([0.0, 1.0], (len(nlay), st.ntargets))
        _, _, err, ymod = st.evaluate_batch(nlay, h, vp, vs, noise, d["site"], rho=rho, want_ymod=True)
        _EXPECTED[kind] = (st, DR.masked(ymod, err, d["site"], st._counts()), err)
    return _EXPECTED[kind]


def check_site(r, st, s, vals, err_s, exact_cols):
    """one site's dict against numpy on its masked synthetics vals [rows, ldy]"""
    ncol = st._counts()
    off = DR.column_blocks(ncol)
    assert r["rows"] == len(vals) and r["failed"] == int((err_s != 0).sum())
    slots = st._slot_rows()[s]
    assert sorted(k for k in r if k not in ("rows", "failed")) == sorted(t.ref for t in slots if t is not None)
    for t, tgt in enumerate(slots):
        if tgt is None:
            continue
        d = r[tgt.ref]
        n = int(ncol[s, t])
        assert bits(d["x"]) == bits(np.asarray(tgt.obsdata.x, float)) and bits(d["obs"]) == bits(np.asarray(tgt.obsdata.y, float))
        assert d["quantiles"].shape == (len(QS), n)
        for j in range(n):
            col = vals[:, off[t] + j]
            w = DR.column_summary(col, QS)
            assert d["count"][j] == w["count"] == len(vals) - int((err_s != 0).sum())
            assert d["nan"][j] == w["nan"] == int((err_s != 0).sum())
            for k in ("min", "max", "median"):
                assert bits(np.float64(d[k][j])) == bits(np.float64(w[k])), (s, tgt.ref, j, k)
            assert bits(d["quantiles"][:, j]) == bits(w["quantiles"]), (s, tgt.ref, j)
            if w["count"] and (off[t] + j) in exact_cols:
                m, var = DR.exact_mean_std(col[~np.isnan(col)])
                assert abs(d["mean"][j] - float(m)) <= 1e-13 * abs(float(m))
                sd = math.sqrt(float(var))
                assert abs(d["std"][j] - sd) <= 1e-13 * sd if var else d["std"][j] == 0.0
            elif not w["count"]:
                assert np.isnan(d["mean"][j]) and np.isnan(d["std"][j])


@pytest.mark.parametrize("kind", ("plain", "one", "missing"))
def test_fill_and_statistics(kind, posterior_rows, engine):
    d = posterior_rows
    mantle = [None, (4.2, 1.8)] * 4 if kind == "plain" else None
    st, vals, err = expected(kind, d, mantle)
    assert sorted(np.flatnonzero(err)) == sorted(np.flatnonzero(d["rows"][:, 0] == 150.0)) and int((err != 0).sum()) == 2
    r = DF._datafits(st, d["rows"], d["vpvs"], site=d["site"], mantle=mantle, engine=engine, batch=1024)
    assert len(r) == len(COUNTS) and [x["rows"] for x in r] == list(COUNTS)
    ldy = vals.shape[1]
    for s in range(len(COUNTS)):
        mine = d["site"] == s
        # (the exact rationals of 8193 values, the site that crosses the 8192-row chunk: both ends of the dispersion block, the
        # first receiver-function column, one in the middle of the first 64-column tile, the tile's last, the next tile's first
        # and last -- every other column goes through the same code with the same chunks; the smaller sites check all of them)
        exact = range(ldy) if COUNTS[s] <= 257 else [q for q in (0, 4, 5, 36, 63, 64, 68) if q < ldy]
        check_site(r[s], st, s, vals[mine], err[mine], set(exact))
    assert r[5]["failed"] == 1 and r[7]["failed"] == 1 and sum(x["failed"] for x in r) == 2
    if kind == "missing":
        assert "prf" not in r[1] and r[2]["rdispph"]["count"].shape == (3,) and r[3]["rdispph"]["count"].shape == (5,)
    if kind == "plain":
        # the same bits on a repeat, from device tensors, with another batch size, in groups of sites, and for a site alone
        import torch
        same(DF._datafits(st, d["rows"], d["vpvs"], site=d["site"], mantle=mantle, engine=engine, batch=1024), r)
        t = lambda a: torch.from_numpy(a).cuda()
        same(DF._datafits(st, t(d["rows"]), t(d["vpvs"]), site=t(d["site"]), mantle=mantle, engine=engine, batch=4096,
                                   max_bytes=300 * 69 * 8), r)
        s = 6
        mine = d["site"] == s
        one = bh.SiteTargets([st.site(s)])
        same(DF.posterior_datafits(one, d["rows"][mine], d["vpvs"][mine], site=np.zeros(COUNTS[s], np.int32), mantle=[mantle[s]],
                                   engine=engine)[0], r[s])


def data_set(st, d, engine, mantle=None, batch=2048):
    """the loaded handle with its DATA set formed (one group)"""
    import torch
    st._register()
    ncol = st._counts()
    ld = DF._DataLoaded(d["rows"], d["site"], engine, st.nsites)
    fw = DF._Forward(engine, torch.device("cuda", 0), batch, d["rows"].shape[1] // 2, st.ntargets, engine.ldy)
    vt = DF._per_row(torch.from_numpy(d["vpvs"]).cuda(), ld.N, "vpvs")
    mv, mk = DF._mantle_arrays(mantle, st.nsites)
    failed = fw.fill(ld, vt, mv, mk, 0, ncol)
    return ld, failed


def test_absent_and_excess_columns_are_masked(posterior_rows, engine):
    """per_site_x="all", missing=True: EVERY column of the DATA set, the ones posterior_datafits leaves out of its dicts
    included, against the restatement -- site 1 lacks the receiver function (columns 5..68), site 2 has 3 periods where the
    block is 5 wide (columns 3, 4): count 0, every row counted as NaN, median and rank keys 0; elsewhere count, NaN count, min,
    max, median and the keys of rank 0 bit for bit"""
    d = posterior_rows
    st, vals, err = expected("missing", d)
    ld, failed = data_set(st, d, engine)
    try:
        stt = ld.scalar_stats(E.SCALARS_DATA)
        S, Q = stt["count"].shape
        assert (S, Q) == (len(COUNTS), 69) and vals.shape[1] == 69
        lo, up = ld.quantile_keys(E.SCALARS_DATA, np.zeros((S, Q, 1), np.uint32))
    finally:
        ld.close()
    masked = 0
    for s in range(S):
        mine = vals[d["site"] == s]
        assert failed[s] == int((err[d["site"] == s] != 0).sum())
        for q in range(Q):
            w = DR.column_summary(mine[:, q])
            assert (stt["count"][s, q], stt["nan"][s, q]) == (w["count"], w["nan"]), (s, q)
            gone = (s == 1 and q >= 5) or (s == 2 and q in (3, 4))
            assert gone == (w["count"] == 0 and COUNTS[s] > 0) or COUNTS[s] == 0, (s, q)
            if not w["count"]:
                assert stt["nan"][s, q] == COUNTS[s]
                assert not stt["median"][s, q].any() and lo[s, q, 0] == 0 and up[s, q, 0] == 0, (s, q)
                masked += gone
                continue
            v = np.sort(mine[:, q][~np.isnan(mine[:, q])])
            assert bits(stt["min"][s, q]) == bits(w["min"]) and bits(stt["max"][s, q]) == bits(w["max"]), (s, q)
            n = w["count"]
            assert bits(stt["med"][s, q]) == bits(np.array([v[(n - 1) // 2], v[min((n - 1) // 2 + 1, n - 1)]])), (s, q)
            assert bits(_keys_to_values(lo[s, q], False)[0]) == bits(v[0]), (s, q)
            assert bits(_keys_to_values(up[s, q], False)[0]) == bits(v[min(1, n - 1)]), (s, q)
    assert masked == 64 + 2
    # what the public call makes of them: the site's dicts hold its own columns only, none of them NaN where rows succeeded
    r = DF.posterior_datafits(st, d["rows"], d["vpvs"], site=d["site"], engine=engine)
    assert "prf" not in r[1] and r[2]["rdispph"]["count"].shape == (3,) and not np.isnan(r[2]["rdispph"]["median"]).any()
    assert np.array_equal(r[2]["rdispph"]["count"], stt["count"][2, :3]) and np.array_equal(r[2]["rdispph"]["nan"], stt["nan"][2, :3])


def check_keys(ld, which, vals_per_site, ranks):
    """lower / upper keys of ranks [S, Q, R] against the sorted values"""
    lo, up = ld.quantile_keys(which, ranks)
    a = _keys_to_values(lo.reshape(-1), False).reshape(lo.shape)
    b = _keys_to_values(up.reshape(-1), False).reshape(up.shape)
    for s, vals in enumerate(vals_per_site):
        for q in range(ranks.shape[1]):
            v = np.sort(vals[:, q][~np.isnan(vals[:, q])])
            for r in range(ranks.shape[2]):
                if not len(v):
                    assert lo[s, q, r] == 0 and up[s, q, r] == 0
                    continue
                k = int(ranks[s, q, r])
                assert bits(a[s, q, r]) == bits(v[k]) and bits(b[s, q, r]) == bits(v[min(k + 1, len(v) - 1)]), (s, q, r, k)


@pytest.mark.parametrize("R", (1, 5, 8))
def test_quantile_keys_of_every_rank(R, posterior_rows, engine):
    """the DATA set (float32-exact dispersion columns and float64 receiver-function columns in one call) and a USER set with a
    constant column; ranks 0, n - 1, two equal ranks in a column, others at random"""
    d = posterior_rows
    st, vals, err = expected("plain", d, [None, (4.2, 1.8)] * 4)
    rs = np.random.RandomState(R)
    ld, failed = data_set(st, d, engine, [None, (4.2, 1.8)] * 4)
    try:
        assert failed.sum() == 2
        stt = ld.scalar_stats(E.SCALARS_DATA)
        cnt = stt["count"]
        f32 = np.array([np.all(vals[:, q][~np.isnan(vals[:, q])].astype(np.float32) == vals[:, q][~np.isnan(vals[:, q])]) for q in range(69)])
        print("float32-exact columns:", np.flatnonzero(f32))
        assert f32[:5].all() and not f32[5:].all()                       # (both key widths in the call)
        S, Q = cnt.shape
        ranks = np.zeros((S, Q, R), np.uint32)
        for s in range(S):
            for q in range(Q):
                n = int(cnt[s, q])
                if n:
                    ranks[s, q] = rs.randint(0, n, R)
                    ranks[s, q, 0] = 0 if (s + q) % 2 else n - 1
                    if R > 1:
                        ranks[s, q, -1] = n - 1 if (s + q) % 2 else 0
                    if R > 2:
                        ranks[s, q, 2] = ranks[s, q, 1]                  # two equal ranks in one column
        per_site = [vals[d["site"] == s] for s in range(S)]
        check_keys(ld, E.SCALARS_DATA, per_site, ranks)
        # the medians of the stats call are ranks like any other
        med = np.maximum(cnt - 1, 0) // 2
        lo, up = ld.quantile_keys(E.SCALARS_DATA, np.repeat(med[:, :, None], R, axis=2).astype(np.uint32))
        assert np.array_equal(lo[:, :, 0], stt["median"][:, :, 0]) and np.array_equal(up[:, :, R - 1], stt["median"][:, :, 1])
        # the USER set: a constant column, a float32 column, a float64 column with NaN
        N = len(d["rows"])
        u = np.stack((np.full(N, 2.5), rs.normal(0, 1, N).astype(np.float32).astype(np.float64), rs.normal(5, 2, N)), axis=1)
        u[rs.randint(0, N, 300), 2] = np.nan
        ld.attach(u, False)
        ucnt = ld.scalar_stats(E.SCALARS_USER)["count"]
        ur = np.zeros((S, 3, R), np.uint32)
        for s in range(S):
            for q in range(3):
                if ucnt[s, q]:
                    ur[s, q] = rs.randint(0, ucnt[s, q], R)
        check_keys(ld, E.SCALARS_USER, [u[d["site"] == s] for s in range(S)], ur)
    finally:
        ld.close()


# ---- end to end -----------------------------------------------------------------------------------------------------------

def chain_targets(nsites=2):
    from test_gpu_sites_priors import full_site
    g = golden("chain_golden.npz")
    return bh.SiteTargets([full_site(g, s, "phase_rf") for s in range(nsites)], names=["st%d" % s for s in range(nsites)],
                          per_site_x="all", per_site_rf=True)


def test_chains_fit_their_device_record(tmp_path, engine):
    """2 sites x 2 chains: the data fits from the device store equal those of the function on the host arrays of samples(), and
    the saved folders give the same best fits"""
    from bayhunter_amd.device_chains import DeviceChains
    from test_gpu_sites_priors import SITE_INIT, SITE_PRIORS
    inits = [dict(SITE_INIT[s], iter_burnin=150, iter_main=150, maxmodels=150, savepath=str(tmp_path))
             for s in range(2)]
    pri = [SITE_PRIORS[0], SITE_PRIORS[2]]                                  # (the second with a mantle rule)
    dc = DeviceChains(chain_targets(), 2, inits, pri, seed=5, search="fast", record="device").run()
    a = dc.posterior_datafits()
    assert len(a) == 2 and all(x["rows"] == 2 * dc.nsamples("p2") for x in a)
    h = dc.samples("p2")
    n, Cn = h["models"].shape[0], h["models"].shape[1]
    m = h["models"].reshape(n * Cn, -1)
    site = np.tile(np.repeat(np.arange(2, dtype=np.int32), 2), n)
    chain = np.tile(np.arange(Cn, dtype=np.int32), n)
    b = DF.posterior_datafits(dc.sites, m, h["vpvs"].reshape(-1), site=site, chain=chain, misfits=h["misfits"][..., -1].reshape(-1),
                              mantle=[p.get("mantle") for p in pri], engine=engine)
    same(a, b)
    for s in range(2):
        assert [x["chain"] for x in a[s]["best"]] == [2 * s, 2 * s + 1] and a[s]["thebest"] in a[s]["best"]
        for x in a[s]["best"]:
            assert x["misfit"] == h["misfits"][..., -1][:, x["chain"]].min() and not np.isnan(x["data"]["prf"]).any()
    # the saved folders: the chain files give the same best fits (no chain is an outlier at dev = 10)
    paths = dc.save(str(tmp_path))
    for p in paths:
        bh.save_final_distribution(p, maxmodels=300, dev=10.0)
    f = bh.datafits_from_storage(paths, dev=10.0, engine=engine)
    for s in range(2):
        assert f[s]["rows"] == a[s]["rows"] and len(f[s]["best"]) == 2
        for x, y in zip(f[s]["best"], a[s]["best"]):
            assert x["chain"] == y["chain"] and x["row"] == y["row"] // Cn and x["misfit"] == y["misfit"] and x["vpvs"] == y["vpvs"]
            assert np.array_equal(x["model"][~np.isnan(x["model"])], y["model"][~np.isnan(y["model"])].astype(np.float64))
            # (the files hold float64 copies of the float32 rows: vp = vs * vpvs is then a float64 product, 6e-8 relative away from
            # the float32 one the device rows give -- the synthetics agree to 1e-5 of their peak, not bit for bit)
            for k in y["data"]:
                assert np.max(np.abs(x["data"][k] - y["data"][k])) <= 1e-5 * np.max(np.abs(y["data"][k])), k
        assert f[s]["thebest"]["chain"] == a[s]["thebest"]["chain"]
    # a station whose saved config lacks the receiver function: the stations become slots, its dispersion numbers stay
    import glob
    import os
    import shutil
    from bayhunter_amd.results import save_config, saved_priors
    alt = str(tmp_path / "st1_swd" / "data")
    shutil.copytree(paths[1], alt)
    cfg = glob.glob(os.path.join(alt, "*_config.pkl"))[0]
    save_config(dc.sites.site(1).targets[:2], cfg, priors=saved_priors(paths[1]), initparams={})
    g = bh.datafits_from_storage([paths[0], alt], dev=10.0, engine=engine)
    assert "prf" in g[0] and "prf" not in g[1] and sorted(g[1]["best"][0]["data"]) == ["ldispph", "rdispph"]
    same(g[0]["prf"], f[0]["prf"])
    for k in ("rdispph", "ldispph"):
        same(g[1][k], f[1][k], (k,))
        same(g[1]["best"][0]["data"][k], f[1]["best"][0]["data"][k])


# ---- defaults -------------------------------------------------------------------------------------------------------------

def test_default_search_and_arithmetic(posterior_rows, engine):
    """the engine's own defaults: the same masks and counts, the dispersion medians within 1e-5 relative of the reference
    search's (the stated tolerance of the short refinement; 9.8e-7 at most was seen here), the receiver-function
    columns bit-equal"""
    d = posterior_rows
    keep = d["site"] < 7                                                   # (without the largest site: a second of forward runs)
    st = site_targets("plain")
    ref = DF.posterior_datafits(st, d["rows"][keep], d["vpvs"][keep], site=d["site"][keep], engine=engine)
    engine.set_swd_search("fast")
    engine.set_swd_arith("fast")
    got = DF.posterior_datafits(st, d["rows"][keep], d["vpvs"][keep], site=d["site"][keep], engine=engine)
    for s in range(len(COUNTS)):
        assert (got[s]["rows"], got[s]["failed"]) == (ref[s]["rows"], ref[s]["failed"])
        assert np.array_equal(got[s]["rdispph"]["count"], ref[s]["rdispph"]["count"])
        same(got[s]["prf"], ref[s]["prf"], (s, "prf"))
        if ref[s]["rows"]:
            a, b = got[s]["rdispph"]["median"], ref[s]["rdispph"]["median"]
            print("site %d: dispersion medians differ by at most %.3g relative" % (s, np.max(np.abs(a - b) / np.abs(b))))
            assert np.all(np.abs(a - b) <= 1e-5 * np.abs(b))


# ---- refusals -------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(posterior_rows, engine):
    import torch
    from bayhunter_amd.posterior import _Loaded
    d = posterior_rows
    rows, site = d["rows"][:500], d["site"][:500]
    L = engine._L
    best = np.full((8, 3), 7, np.int64)
    lo, up = np.full(8 * 2 * 9, 7, np.uint64), np.full(8 * 2 * 9, 7, np.uint64)
    dbuf = torch.zeros(64 * 24, dtype=torch.float64).cuda()
    ibuf = torch.zeros(64, dtype=torch.int32).cuda()
    dp, ip = C.c_void_p(dbuf.data_ptr()), C.c_void_p(ibuf.data_ptr())
    vp_host = np.full(500, 1.7)

    def refused(rc, text):
        with pytest.raises(E.EngineError, match=text):
            engine._check(rc)
        assert (best == 7).all() and (lo == 7).all() and (up == 7).all() and not dbuf.any() and not ibuf.any()

    chain = np.zeros(500, np.int32)
    mis = np.ones(500)
    plain = _Loaded(rows, site, engine, 8)                                 # rows loaded without bh_posterior_keep_rows
    try:
        refused(L.bh_posterior_layers(plain._p, 0, 64, E.HOST, None, 8, 1, _ptr(vp_host), None, None, ip, dp, dp, dp, dp, 64, ip),
                "bh_posterior_keep_rows")
        refused(L.bh_posterior_best(plain._p, 3, E.HOST, None, _ptr(chain), 1, 8, _ptr(mis), 1, _ptr(best), None), "bh_posterior_keep_rows")
        refused(L.bh_posterior_data_fill(plain._p, None, 0, 0, 1, None, None, 1, _ptr(np.ones((8, 1), np.int32)), None),
                "bh_posterior_keep_rows")
    finally:
        plain.close()
    ld = DF._DataLoaded(rows, site, engine, 8)
    try:
        # an unformed set
        rk = np.zeros((8, 2, 1), np.uint32)
        refused(L.bh_posterior_scalar_quantiles(ld._p, E.SCALARS_DATA, 1, _ptr(rk), _ptr(lo), _ptr(up)), "does not exist yet")
        refused(L.bh_posterior_scalar_cols(ld._p, E.SCALARS_DATA, _ptr(np.zeros(1, np.int32))), "DATA set does not exist yet")
        refused(L.bh_posterior_scalar_quantiles(ld._p, 2, 1, _ptr(rk), _ptr(lo), _ptr(up)), "no such scalar set")
        # a chain id out of range (host ids are checked before anything is launched), NaN misfits
        bad = chain.copy()
        bad[17] = 3
        refused(L.bh_posterior_best(ld._p, 3, E.HOST, None, _ptr(bad), 1, 8, _ptr(mis), 1, _ptr(best), None), "chain id out of range")
        bad[17] = -1
        refused(L.bh_posterior_best(ld._p, 3, E.HOST, None, _ptr(bad), 1, 8, _ptr(mis), 1, _ptr(best), None), "chain id out of range")
        nanmis = mis.copy()
        nanmis[3] = np.nan
        refused(L.bh_posterior_best(ld._p, 3, E.HOST, None, _ptr(chain), 1, 8, _ptr(nanmis), 1, _ptr(best), None), "NaN")
        refused(L.bh_posterior_best(ld._p, 0, E.HOST, None, _ptr(chain), 1, 8, _ptr(mis), 1, _ptr(best), None), "nchains")
        # Q > BH_DATAFIT_MAXCOLS, blocks that do not add up, calls out of order
        nc = np.ones((8, 1), np.int32)
        refused(L.bh_posterior_data_fill(ld._p, None, 0, 0, E.DATAFIT_MAXCOLS + 1, dp, ip, 1, _ptr(nc), None), "BH_DATAFIT_MAXCOLS")
        refused(L.bh_posterior_data_fill(ld._p, None, 0, 0, 2, dp, ip, 1, _ptr(nc), None), "add up")
        refused(L.bh_posterior_data_fill(ld._p, None, 64, 64, 1, dp, ip, 1, _ptr(nc), None), "in order")
        refused(L.bh_posterior_layers(ld._p, 0, ld.nrows + 1, E.HOST, None, 8, 1, _ptr(vp_host), None, None, ip, dp, dp, dp, dp, 1024, ip),
                "not among the loaded rows")
        refused(L.bh_posterior_layers(ld._p, 0, 64, E.HOST, None, 8, 1, _ptr(vp_host), None, None, ip, dp, dp, dp, dp, 63, ip), "stride_l")
        # R = 0, R > 8, a rank >= the column's count, stats not run: on a formed USER set
        u = np.stack((np.arange(500.0), np.full(500, np.nan)), axis=1)
        ld.attach(u, False)
        refused(L.bh_posterior_scalar_quantiles(ld._p, E.SCALARS_USER, 1, _ptr(rk), _ptr(lo), _ptr(up)), "bh_posterior_scalar_stats")
        cnt = ld.scalar_stats(E.SCALARS_USER)["count"]
        assert cnt[:, 1].sum() == 0 and cnt[:, 0].sum() == 500
        refused(L.bh_posterior_scalar_quantiles(ld._p, E.SCALARS_USER, 0, _ptr(rk), _ptr(lo), _ptr(up)), "BH_QUANTILES_MAXRANKS")
        refused(L.bh_posterior_scalar_quantiles(ld._p, E.SCALARS_USER, 9, _ptr(np.zeros((8, 2, 9), np.uint32)), _ptr(lo), _ptr(up)),
                "BH_QUANTILES_MAXRANKS")
        over = rk.copy()
        s = int(np.argmax(cnt[:, 0]))
        over[s, 0, 0] = cnt[s, 0]
        refused(L.bh_posterior_scalar_quantiles(ld._p, E.SCALARS_USER, 1, _ptr(over), _ptr(lo), _ptr(up)), "not below")
        over = rk.copy()
        over[s, 1, 0] = 1                                                 # (an empty column takes rank 0 only)
        refused(L.bh_posterior_scalar_quantiles(ld._p, E.SCALARS_USER, 1, _ptr(over), _ptr(lo), _ptr(up)), "not below")
        refused(L.bh_posterior_scalar_gather(ld._p, E.SCALARS_USER, 1, _ptr(np.array([ld.nrows], np.int64)), _ptr(np.zeros(2))), "position")
        # the same handle still works
        over[s, 1, 0] = 0
        over[s, 0, 0] = cnt[s, 0] - 1
        l2, u2 = ld.quantile_keys(E.SCALARS_USER, over)
        assert _keys_to_values(l2[s, 0], False)[0] == u[site == s, 0].max() and l2[s, 0, 0] == u2[s, 0, 0] and l2[s, 1, 0] == 0
    finally:
        ld.close()
