"""Per-site posteriors of Moho depth, crustal vs and scalar columns on the GPU (bayhunter_amd/posterior.py,
include/bh_engine_posterior_scalars.h) against the restatement tests/moho_ref.py, which tests/test_moho_ref.py holds to the
reference's own outputs: bit for bit for counts, min, max, medians, edges, histograms and modes; mean and std within 1e-13 of
the exact rationals."""
import math

import numpy as np
import pytest

from conftest import golden
import moho_ref as MR

pytestmark = pytest.mark.gpu
KEYS = ("f32", "f64of32", "f64")
STATS = ("median", "mean", "std", "min", "max")


@pytest.fixture(scope="module")
def G():
    return golden("moho_golden.npz")


def same(a, b, what=()):
    """nested dicts / tuples / lists / arrays / numbers: the same keys, dtypes and bits (NaN equal to NaN)"""
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), what
        for k in a:
            same(a[k], b[k], what + (k,))
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, what + (i,))
    else:
        x, y = np.asarray(a), np.asarray(b)
        assert x.dtype == y.dtype and x.shape == y.shape, what
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), what


def check_exact(d, v):
    """mean and std of a statistics dict against the exact rationals of the values v"""
    m, var = MR.exact_mean_std(v)
    assert abs(d["mean"] - float(m)) <= 1e-13 * abs(float(m))
    if var == 0:
        assert d["std"] == 0.0
    else:
        s = math.sqrt(float(var))
        assert abs(d["std"] - s) <= 1e-13 * s


_ROWS = {}


def cached_rows(models, lo, hi, mv):
    """the restated rows of a set, computed once (the tests share their sets)"""
    key = (models.ctypes.data, models.shape, models.dtype.str, float(lo), float(hi), float(mv))
    if key not in _ROWS:
        _ROWS[key] = (models, MR.moho_rows(models, lo, hi, mv))    # (the set is kept alive with its rows)
    return _ROWS[key][1]


def check_moho(r, models, lo, hi, mv, bins=50, exact=True):
    s = MR.moho_summary(models, lo, hi, mv, bins, rows=cached_rows(models, lo, hi, mv))
    assert (r["rows"], r["count"]) == (s["rows"], s["count"])
    if not s["count"]:
        empty = np.histogram_bin_edges(np.zeros(0), bins)
        for name in MR.COLUMNS:
            assert all(np.isnan(r[name][k]) for k in STATS)
            assert not r["hist"][name][0].any() and np.array_equal(r["hist"][name][1], empty)
        for name in MR.COLUMNS[1:]:
            assert not r["hist2d"][name][0].any() and r["hist2d"][name][0].shape == (bins, bins)
            assert np.isnan(r["mode"][name]).all()
        return s
    for q, name in enumerate(MR.COLUMNS):
        for k in ("median", "min", "max"):
            assert r[name][k] == s[name][k], (name, k)
        same(r["hist"][name], (s["hist"][name][0].astype(np.int64), s["hist"][name][1]), (name, "hist"))
        if exact:
            check_exact(r[name], s["values"][:, q])
    for name in MR.COLUMNS[1:]:
        same(r["hist2d"][name], (s["hist2d"][name][0].astype(np.int64),) + s["hist2d"][name][1:], (name, "hist2d"))
        assert r["mode"][name] == s["mode"][name]
    return s


def check_scalar(d, v, bins=20, nlayer_edges=False, exact=True, live=False):
    """one column's statistics against the restatement (live: against numpy's own histogram and median of the column)"""
    s = MR.scalar_summary(v, bins, nlayer_edges)
    assert (d["count"], d["nan"]) == (s["count"], s["nan"])
    if not s["count"]:
        assert all(np.isnan(d[k]) for k in STATS) and not d["hist"][0].any() and np.isnan(d["mode"]) and not d["constant"]
        return
    x = np.asarray(v)[~np.isnan(v)]
    for k in ("median", "min", "max", "mode", "constant"):
        assert d[k] == s[k] and np.asarray(d[k]).dtype == np.asarray(s[k]).dtype, k
    same(d["hist"], (s["hist"][0].astype(np.int64), s["hist"][1]), ("hist",))
    if live and not s["constant"]:
        c, e = np.histogram(x, bins)
        assert np.array_equal(d["hist"][0], c) and np.array_equal(d["hist"][1], e) and d["hist"][1].dtype == e.dtype
        m = np.median(x)
        assert d["median"] == m and type(d["median"]) is type(m)
    if exact:
        check_exact(d, x)


# ---- golden sets ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", KEYS)
def test_golden_moho_sets_are_the_references(G, key, engine):
    from bayhunter_amd import posterior_moho
    m = G[key + "_models"]
    lo, hi, mv, bins = float(G["lo"]), float(G["hi"]), float(G["mohovs"]), int(G["bins"])
    r = posterior_moho(m, moho=(lo, hi), mohovs=mv, bins=bins, engine=engine)
    check_moho(r, m, lo, hi, mv, bins)
    v = G[key + "_values"]
    assert r["count"] == len(v) and r["invalid_rows"] == 0 and r["dropped"] == 0
    for q, name in enumerate(MR.COLUMNS):
        assert r[name]["median"] == G[key + "_medians"][q]
        assert (r[name]["min"], r[name]["max"]) == (v[:, q].min(), v[:, q].max())
        assert np.array_equal(r["hist"][name][0], G[key + "_hist"][q])
    for i, name in enumerate(MR.COLUMNS[1:]):
        assert np.array_equal(r["hist2d"][name][0], G[key + "_hist2d"][i])


def golden_columns(G, dtype):
    return dict(likes=G["sc_likes"].astype(dtype), misfits=G["sc_misfits"].astype(dtype), vpvs=G["sc_vpvs"].astype(dtype),
                noise=G["sc_noise"].astype(dtype))


def test_golden_scalar_columns_are_the_references(G, engine):
    from bayhunter_amd import posterior_scalars
    m = G["sc_models"]
    cols = golden_columns(G, np.float64)
    r = posterior_scalars(m, cols, engine=engine)
    assert r["rows"] == len(m)
    for key, d, v in [("likes_0", r["likes"], cols["likes"]), ("vpvs_0", r["vpvs"], cols["vpvs"]),
                      ("others_1", r["misfits"][2], cols["misfits"][:, 2])] + \
                     [("misfits_%d" % i, r["misfits"][i], cols["misfits"][:, i]) for i in range(2)] + \
                     [("noise_%d" % i, r["noise"][i], cols["noise"][:, i]) for i in range(4)]:
        check_scalar(d, v)
        assert np.array_equal(d["hist"][0], G["sc_%s_hist" % key]) and d["median"] == float(G["sc_%s_median" % key]), key
        assert d["constant"] == (key in ("noise_0", "noise_2"))
        if d["constant"]:
            assert d["std"] == 0.0 and d["mean"] == d["min"]
    check_scalar(r["nlayers"], MR.nlayers(m), nlayer_edges=True)
    assert np.array_equal(r["nlayers"]["hist"][0], G["sc_nlayers_0_hist"])
    assert r["nlayers"]["median"] == float(G["sc_nlayers_0_median"])


def test_float32_scalar_columns_are_numpys(G, engine):
    from bayhunter_amd import posterior_scalars
    m = G["sc_models"].astype(np.float32)
    keep = np.ones(len(m), bool)
    keep[::7] = False
    m[~keep] = np.nan                                                 # rows of NaN only: their values are ignored
    cols = golden_columns(G, np.float32)
    r = posterior_scalars(m, cols, engine=engine)
    for d, v in [(r["likes"], cols["likes"]), (r["vpvs"], cols["vpvs"])] + [(r["misfits"][i], cols["misfits"][:, i]) for i in range(3)] + \
                [(r["noise"][i], cols["noise"][:, i]) for i in range(4)]:
        check_scalar(d, v[keep], live=True)
        assert type(d["median"]) is np.float32
    # float32 and float64 columns in one call keep their own dtype rules
    mixed = posterior_scalars(m, dict(likes=cols["likes"], vpvs=G["sc_vpvs"]), nlayers=False, engine=engine)
    same(mixed["likes"], r["likes"])
    check_scalar(mixed["vpvs"], G["sc_vpvs"][keep], live=True)
    assert "nlayers" not in mixed


# ---- sites ------------------------------------------------------------------------------------------------------------

def crust_rows(rs, N, ML=12, dtype=np.float32):
    """rows of a slow crust over a fast mantle, 2..ML layers, and a few of any kind"""
    rows = np.full((N, 2 * ML), np.nan)
    for i in range(N):
        n = rs.randint(2, ML + 1)
        nc = rs.randint(1, n)
        z = np.sort(rs.uniform(0, 60, n))
        vs = np.concatenate((rs.uniform(2.0, 4.1, nc), rs.uniform(3.9, 4.8, n - nc)))
        rows[i, :n], rows[i, n:2 * n] = vs, z
    return rows.astype(dtype)


@pytest.fixture(scope="module")
def site_set():
    """65 sites with their own (lo, hi, mohovs); site 5 spans two chunks of 8192 rows, site 7 has no Moho row, site 9 exactly one"""
    rs = np.random.RandomState(65)
    S = 65
    per = [crust_rows(rs, 8300 if s == 5 else 40 + 3 * s, dtype=(np.float32 if s % 2 else np.float64)).astype(np.float64)
           for s in range(S)]
    per[3] = per[3] + rs.uniform(-1e-7, 1e-7, per[3].shape)             # one site of general float64 values
    per[7][:, 0] = 2.0
    per[7][:, 1:12] = np.minimum(per[7][:, 1:12], 3.0)                   # nothing above mohovs
    one = np.full((30, 24), np.nan)
    one[:, 0], one[:, 1] = 3.0, rs.uniform(0, 50, 30)                    # one-layer rows ...
    one[11, :4] = 3.5, 4.6, 10.0, 50.0                                   # ... and one Moho at 30 km
    per[9] = one
    lo = rs.uniform(0, 15, S)
    lo[2] = 0.0
    hi = lo + rs.uniform(20, 40, S)
    mv = rs.uniform(3.9, 4.3, S)
    lo[9], hi[9], mv[9] = 5.0, 45.0, 4.2
    rows = np.concatenate(per)
    site = np.concatenate([np.full(len(p), s, np.int32) for s, p in enumerate(per)])
    like = rs.normal(0, 1, len(rows)).astype(np.float32)
    perm = rs.permutation(len(rows))
    return dict(S=S, per=per, lo=lo, hi=hi, mv=mv, rows=rows[perm], site=site[perm], like=like[perm], perm=perm,
                like_per=[like[site == s] for s in range(S)])


def test_sites_among_others_alone_and_again(site_set, engine):
    from bayhunter_amd import posterior_moho, posterior_scalars
    d = site_set
    moho = np.stack((d["lo"], d["hi"]), axis=1)
    a = posterior_moho(d["rows"], site=d["site"], moho=moho, mohovs=d["mv"], engine=engine)
    b = posterior_moho(d["rows"], site=d["site"], moho=moho, mohovs=d["mv"], engine=engine)
    same(a, b)
    assert len(a) == d["S"] and a[5]["rows"] == 8300 and a[5]["count"] > 3000
    assert a[7]["rows"] == len(d["per"][7]) and a[7]["count"] == 0 and a[9]["count"] == 1
    assert a[9]["moho"] == dict(median=30.0, mean=30.0, std=0.0, min=30.0, max=30.0) and a[9]["vsjump"]["median"] == 4.6 - 3.5
    for s in (0, 3, 5, 7, 9, 64):
        alone = posterior_moho(d["per"][s], moho=(d["lo"][s], d["hi"][s]), mohovs=d["mv"][s], engine=engine)
        same(alone, a[s], (s,))
        check_moho(a[s], d["per"][s], d["lo"][s], d["hi"][s], d["mv"][s], exact=s != 5)
    for s in range(10, 64, 9):
        check_moho(a[s], d["per"][s], d["lo"][s], d["hi"][s], d["mv"][s], exact=False)
    v = cached_rows(d["per"][5], d["lo"][5], d["hi"][5], d["mv"][5])
    check_exact(a[5]["vscrust"], v[~np.isnan(v[:, 2]), 2])                # the exact sums across chunks (one column of the four)
    # a scalar column follows its rows through the same permutation
    c = posterior_scalars(d["rows"], dict(like=d["like"]), site=d["site"], engine=engine)
    same(c, posterior_scalars(d["rows"], dict(like=d["like"]), site=d["site"], engine=engine))
    for s in (0, 5, 9, 64):
        same(posterior_scalars(d["per"][s], dict(like=d["like_per"][s]), engine=engine), c[s], (s,))
        check_scalar(c[s]["like"], d["like_per"][s], live=True, exact=s != 5)
        check_scalar(c[s]["nlayers"], MR.nlayers(d["per"][s]), nlayer_edges=True, exact=False)
    # one pair and one mohovs spread over every site
    e = posterior_moho(d["rows"], site=d["site"], moho=(5.0, 45.0), engine=engine)
    check_moho(e[12], d["per"][12], 5.0, 45.0, 4.2)


def test_histograms_on_both_sides_of_the_lds_limits(site_set, engine):
    """1-D: 2048 bins of a site stay in LDS, 2049 go to global atomics; 2-D: 64 x 64 cells stay, 65 x 65 go"""
    from bayhunter_amd import posterior_moho, posterior_scalars
    d = site_set
    s = 5
    for bins in (64, 65):
        r = posterior_moho(d["per"][s], moho=(d["lo"][s], d["hi"][s]), mohovs=d["mv"][s], bins=bins, engine=engine)
        check_moho(r, d["per"][s], d["lo"][s], d["hi"][s], d["mv"][s], bins=bins, exact=False)
    for bins in (2048, 2049):
        r = posterior_scalars(d["per"][s], dict(like=d["like_per"][s]), bins=bins, nlayers=False, engine=engine)
        check_scalar(r["like"], d["like_per"][s], bins=bins, live=True, exact=False)


# ---- device path ------------------------------------------------------------------------------------------------------

def test_device_tensors_equal_the_host_path(engine):
    import torch
    from bayhunter_amd import posterior_moho, posterior_scalars
    rs = np.random.RandomState(4)
    for dt in (np.float32, np.float64):
        m = crust_rows(rs, 5000, dtype=dt)
        m[5, 3] = np.nan                                              # not a prefix: left out and counted on the device path
        site = rs.randint(0, 4, len(m)).astype(np.int32)
        site[rs.randint(0, len(m), 300)] = -1                         # rows that are no samples
        site[5] = 2
        val = rs.normal(5, 2, (len(m), 3)).astype(dt)
        val[rs.randint(0, len(m), 100), 1] = np.nan
        wide_m = torch.full((len(m), m.shape[1] + 5), 7.0, dtype=torch.from_numpy(m).dtype).cuda()
        wide_m[:, :m.shape[1]] = torch.from_numpy(m).cuda()
        wide_v = torch.full((len(m), 8), -3.0, dtype=wide_m.dtype).cuda()
        wide_v[:, 2:5] = torch.from_numpy(val).cuda()
        mt, vt, st = wide_m[:, :m.shape[1]], wide_v[:, 2:5], torch.from_numpy(site).cuda()
        assert mt.stride(0) == m.shape[1] + 5 and vt.stride(0) == 8
        good = site >= 0
        good[5] = False
        moho = [(0.0, 40.0), (5.0, 50.0), (10.0, 45.0), (2.0, 30.0)]
        a = posterior_moho(mt, site=st, moho=moho, mohovs=4.1, engine=engine, nsites=4)
        b = posterior_moho(m[good], site=site[good], moho=moho, mohovs=4.1, engine=engine, nsites=4)
        c = posterior_scalars(mt, dict(v=vt, w=vt[:, 0]), site=st, engine=engine, nsites=4)
        e = posterior_scalars(m[good], dict(v=val[good], w=val[good, 0]), site=site[good], engine=engine, nsites=4)
        nbad = int((site < 0).sum())
        for s in range(4):
            assert a[s]["dropped"] == c[s]["dropped"] == nbad and b[s]["dropped"] == 0
            assert a[s]["invalid_rows"] == c[s]["invalid_rows"] == (1 if s == 2 else 0)
            for x in (a[s], c[s]):
                x.pop("dropped"), x.pop("invalid_rows")
            for x in (b[s], e[s]):
                x.pop("dropped"), x.pop("invalid_rows")
            same(a[s], b[s], (s, "moho"))
            same(c[s], e[s], (s, "scalars"))
            mine = good & (site == s)
            assert c[s]["v"][1]["nan"] == int(np.isnan(val[mine, 1]).sum()) > 0
            assert c[s]["v"][1]["count"] + c[s]["v"][1]["nan"] == c[s]["rows"] == int(mine.sum())
            check_scalar(c[s]["v"][1], val[mine, 1], live=True, exact=False)
            check_moho(a[s], m[mine], moho[s][0], moho[s][1], 4.1, exact=False)


# ---- chains -----------------------------------------------------------------------------------------------------------

def chain_columns(h, n):
    return dict(likes=h["likes"].reshape(n), vpvs=h["vpvs"].reshape(n), misfits=h["misfits"].reshape(n, -1),
                noise=h["noise"].reshape(n, -1))


def site_targets(nsites=2):
    import bayhunter_amd as bh
    from test_gpu_sites_priors import full_site
    g = golden("chain_golden.npz")
    return bh.SiteTargets([full_site(g, s, "phase_rf") for s in range(nsites)], names=["st%d" % s for s in range(nsites)],
                          per_site_x="all", per_site_rf=True)


def test_chains_summarise_their_device_record(engine):
    """2 sites x 8 chains under their own priors, every iteration kept: the summaries from the device store equal those of the
    functions on the host arrays of samples(site=s), whose rows have the site's own width"""
    from bayhunter_amd import posterior_moho, posterior_scalars
    from bayhunter_amd.device_chains import DeviceChains
    from test_gpu_sites_priors import SITE_INIT, SITE_PRIORS
    inits = [dict(SITE_INIT[s], iter_burnin=200, iter_main=200, maxmodels=200) for s in range(2)]
    dc = DeviceChains(site_targets(), 8, inits, SITE_PRIORS[:2], seed=78, search="fast", record="device").run()
    assert dc.thinning == 1 and dc.nsamples("p2") == 200
    mv = [3.6, 3.8]
    a = dc.posterior_moho(mohovs=mv)                                   # every site's own priors['z']
    b = dc.posterior_moho(moho=(3.0, 40.0), mohovs=mv, exclude_chains=(1, 9, 10))
    c = dc.posterior_scalars()
    assert sum(x["count"] for x in a) > 0
    for s in range(2):
        h = dc.samples("p2", site=s)
        n = 200 * 8
        m = h["models"].reshape(n, -1)
        assert m.shape[1] == 2 * (SITE_PRIORS[s]["layers"][1] + 1) and a[s]["rows"] == n and a[s]["dropped"] == 0
        same(a[s], posterior_moho(m, moho=SITE_PRIORS[s]["z"], mohovs=mv[s], engine=engine), (s, "moho"))
        same(c[s], posterior_scalars(m, chain_columns(h, n), engine=engine), (s, "scalars"))
        keep = np.ones(8, bool)
        keep[[1] if s == 0 else [1, 2]] = False                        # chains 1 | 9, 10
        mk = h["models"][:, keep].reshape(200 * keep.sum(), -1)
        want = posterior_moho(mk, moho=(3.0, 40.0), mohovs=mv[s], engine=engine)
        assert b[s]["dropped"] == 3 * 200 and b[s]["rows"] == len(mk)
        b[s].pop("dropped"), want.pop("dropped")
        same(b[s], want, (s, "excluded"))
    host = DeviceChains(site_targets(), 8, inits, SITE_PRIORS[:2], seed=78, search="fast", record="host")
    with pytest.raises(Exception, match="record='device'"):
        host.posterior_moho()
    with pytest.raises(Exception, match="record='device'"):
        host.posterior_scalars()


def test_tempered_chains_summarise_their_cold_rows(engine):
    """one ladder of 4 temperatures per site: the beta = 1 rows are selected on the device"""
    from bayhunter_amd import posterior_moho, posterior_scalars
    from bayhunter_amd.device_chains import DeviceChains
    from test_gpu_chains import SETUPS
    su = SETUPS["exp"]
    init = dict(su["init"], iter_burnin=280, iter_main=120, maxmodels=120)
    ladder = np.repeat(np.arange(2), 4)
    betas = np.tile(1.0 / np.geomspace(1.0, 20.0, 4), 2)
    dc = DeviceChains(site_targets(), 4, init, su["priors"], seed=6, betas=betas, ladder=ladder, swap_every=20,
                      record="device").run()
    assert dc.nswaps > 0 and dc.thinning == 1
    d = dc.samples_dev("p2", cold_only=True)
    beta = dc.samples("p2")["beta"]
    assert not np.all(beta[:, 0] == 1.0)                                # (the cold chain moved)
    assert np.array_equal(d["site"].cpu().numpy().reshape(120, 8) >= 0, beta == 1.0)
    a, c = dc.posterior_moho(mohovs=3.7), dc.posterior_scalars()        # cold_only by default
    every = dc.posterior_moho(mohovs=3.7, cold_only=False)
    for s in range(2):
        h = dc.samples("p2", cold_only=True, site=s)
        assert h["models"].shape[:2] == (120, 1) and np.all(h["beta"] == 1.0)
        m = h["models"].reshape(120, -1)
        assert a[s]["rows"] == 120 and a[s]["dropped"] == 2 * 3 * 120 and every[s]["rows"] == 480
        want = posterior_moho(m, moho=su["priors"]["z"], mohovs=3.7, engine=engine)
        wc = posterior_scalars(m, chain_columns(h, 120), engine=engine)
        for x in (a[s], c[s], want, wc):
            x.pop("dropped")
        same(a[s], want, (s, "moho"))
        same(c[s], wc, (s, "scalars"))


def test_moho_from_storage_reads_every_stations_files_and_saved_range(tmp_path, engine):
    import bayhunter_amd as bh
    from bayhunter_amd.results import save_config
    rs = np.random.RandomState(12)
    sets = [crust_rows(rs, 300, ML=12, dtype=np.float32).astype(np.float64), crust_rows(rs, 200, ML=6, dtype=np.float32).astype(np.float64)]
    ranges = [(5, 45), (0.0, 38.5)]
    paths = []
    for s, (m, z) in enumerate(zip(sets, ranges)):
        d = tmp_path / ("st%d" % s) / "data"
        d.mkdir(parents=True)
        np.save(str(d / "c_models.npy"), m)
        save_config([], str(d / ("st%d_config.pkl" % s)), priors=dict(z=z, vs=(2, 5)), initparams={})
        paths.append(str(d))
    r = bh.moho_from_storage(paths, mohovs=4.1, engine=engine)
    for s in range(2):
        assert r[s]["count"] > 50
        same(r[s], bh.posterior_moho(sets[s], moho=ranges[s], mohovs=4.1, engine=engine), (s,))
        check_moho(r[s], sets[s], ranges[s][0], ranges[s][1], 4.1, exact=False)
    same(bh.moho_from_storage(paths, moho=(2.0, 30.0), engine=engine)[1], bh.posterior_moho(sets[1], moho=(2.0, 30.0), engine=engine))


# ---- refusals ---------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(engine):
    import ctypes as C
    from bayhunter_amd import engine as E
    from bayhunter_amd import posterior_moho
    from bayhunter_amd.posterior import _Loaded, _ptr
    rs = np.random.RandomState(9)
    m = crust_rows(rs, 200)
    with pytest.raises(E.EngineError, match="below 0"):
        posterior_moho(m, moho=(-1.0, 40.0), engine=engine)
    with pytest.raises(E.EngineError, match="lo < hi"):
        posterior_moho(m, moho=(30.0, 30.0), engine=engine)
    plain = _Loaded(m, None, engine)                                   # rows loaded without bh_posterior_keep_rows
    try:
        with pytest.raises(E.EngineError, match="bh_posterior_keep_rows"):
            plain.moho([0.0], [60.0], [4.0])
        with pytest.raises(E.EngineError, match="bh_posterior_keep_rows"):
            plain.attach(None, True)
        assert plain.columns(np.array([0.0, 10.0]))["min"].shape == (1, 2)   # (the handle serves the column passes as before)
    finally:
        plain.close()
    ld = _Loaded(m, None, engine, scalars=True)
    L = ld._L
    cnt, am = np.zeros(1 << 12, np.uint32), np.zeros(1, np.int64)
    off = np.array([0, 3], np.int64)
    ok, desc = np.array([0.0, 1.0, 2.0]), np.array([0.0, 2.0, 1.0])

    def refused(rc, text):
        with pytest.raises(E.EngineError, match=text):
            engine._check(rc)
        assert not cnt.any()

    try:
        # a set that does not exist yet
        refused(L.bh_posterior_scalar_hist(ld._p, E.SCALARS_MOHO, 0, _ptr(off), _ptr(ok), _ptr(cnt)), "does not exist yet")
        refused(L.bh_posterior_scalar_hist(ld._p, E.SCALARS_USER, 0, _ptr(off), _ptr(ok), _ptr(cnt)), "does not exist yet")
        refused(L.bh_posterior_scalar_cols(ld._p, E.SCALARS_USER, _ptr(np.zeros(1, np.int32))), "does not exist yet")
        refused(L.bh_posterior_scalar_hist(ld._p, 2, 0, _ptr(off), _ptr(ok), _ptr(cnt)), "no such scalar set")
        assert ld.moho([0.0], [60.0], [4.0])[0] > 0
        # a column out of range
        refused(L.bh_posterior_scalar_hist(ld._p, E.SCALARS_MOHO, 4, _ptr(off), _ptr(ok), _ptr(cnt)), "column out of range")
        refused(L.bh_posterior_scalar_hist2d(ld._p, E.SCALARS_MOHO, 1, -1, _ptr(off), _ptr(ok), _ptr(off), _ptr(ok), _ptr(cnt),
                                             _ptr(am)), "column out of range")
        # edges that are not ascending, too few edges
        refused(L.bh_posterior_scalar_hist(ld._p, E.SCALARS_MOHO, 0, _ptr(off), _ptr(desc), _ptr(cnt)), "ascending")
        refused(L.bh_posterior_scalar_hist2d(ld._p, E.SCALARS_MOHO, 1, 0, _ptr(off), _ptr(ok), _ptr(off), _ptr(desc), _ptr(cnt),
                                             _ptr(am)), "ascending")
        refused(L.bh_posterior_scalar_hist(ld._p, E.SCALARS_MOHO, 0, _ptr(np.array([0, 1], np.int64)), _ptr(ok), _ptr(cnt)), "edges")
        # more cells than the cap: 2^14 x 2^14 = 2^28 cells
        big = np.arange((1 << 14) + 1, dtype=np.float64)
        boff = np.array([0, big.size], np.int64)
        refused(L.bh_posterior_scalar_hist2d(ld._p, E.SCALARS_MOHO, 1, 0, _ptr(boff), _ptr(big), _ptr(boff), _ptr(big), _ptr(cnt),
                                             _ptr(am)), "BH_POSTERIOR_MAXCOUNTS")
        # the Moho range
        for lo, hi, text in ((-0.5, 10.0, "below 0"), (10.0, 10.0, "lo < hi"), (10.0, 5.0, "lo < hi"), (0.0, np.inf, "finite")):
            with pytest.raises(E.EngineError, match=text):
                ld.moho([lo], [hi], [4.2])
            # (a refused bh_posterior_moho leaves the set as it was)
            q = np.zeros(1, np.int32)
            engine._check(L.bh_posterior_scalar_cols(ld._p, E.SCALARS_MOHO, _ptr(q)))
            assert q[0] == 4
        # attach: too many columns, nothing to attach
        with pytest.raises(E.EngineError, match="BH_SCALARS_MAXCOLS"):
            ld.attach(np.zeros((200, 65), np.float32), False)
        with pytest.raises(E.EngineError, match="no column"):
            ld.attach(None, False)
        # the same handle still works
        assert ld.scalar_hist(E.SCALARS_MOHO, 0, [np.array([0.0, 30.0, 60.0])])[0].sum() == ld.moho([0.0], [60.0], [4.0])[0]
    finally:
        ld.close()
