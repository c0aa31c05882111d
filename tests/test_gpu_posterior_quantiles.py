"""Credible intervals on the GPU (include/bh_engine_posterior_quantiles.h; bayhunter_amd/posterior.py: quantiles= of posterior_models,
posterior_moho and posterior_scalars; DeviceChains.posterior_models / posterior_hist2d) against numpy.quantile(...,
method="linear") of the restated columns (tests/posterior_ref.interp, tests/moho_ref): every comparison is on bits."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
import moho_ref as MR
import posterior_ref as R
from test_posterior_quantiles_host import okeys

pytestmark = pytest.mark.gpu
KEYS = ("f32", "f64of32", "f64")
Q5 = (0.025, 0.16, 0.5, 0.84, 0.975)
QLISTS = dict(q1=(0.5,), q2=(0.0, 1.0), q5=Q5, q8=(0.01, 0.1, 0.25, 0.4, 0.6, 0.75, 0.9, 0.99),
              q9=(0.0, 0.05, 0.2, 1 / 3., 0.5, 2 / 3., 0.8, 0.95, 1.0), q17=tuple(np.linspace(0, 1, 17)),
              qdup=(0.5, 0.5, 0.1, 0.5), quns=(0.9, 0.1, 0.6, 0.3))
MODEL_KEYS = {"count", "invalid_rows", "mode_valid", "mean", "median", "minmax", "stdminmax", "mode"}
STAT_KEYS = {"median", "mean", "std", "min", "max"}
SCALAR_KEYS = STAT_KEYS | {"count", "nan", "constant", "hist", "mode"}
FILL = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def G():
    return golden("posterior_golden.npz")


def ptr(a):
    return C.c_void_p(a.ctypes.data)


def bits_equal(a, b):
    """the same shape, NaN in the same places, the same bits elsewhere"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a.view(np.uint64)[ok], b.view(np.uint64)[ok])


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


def synth(rs, N, ML, kind, ties=False):
    """rows of 1..ML layers (ragged; every seventh row has one layer, row 1 has ML): kind f32 = float32 rows, f64of32 = float64
    rows of float32-exact vs, f64 = float64 rows whose vs are not float32-exact; ties: vs in multiples of 0.25"""
    n = rs.randint(1, ML + 1, N)
    n[::7] = 1
    if N > 1:
        n[1] = ML
    vs = rs.uniform(2.0, 4.8, (N, ML))
    if ties:
        vs = np.round(vs * 4) / 4
    vs = vs.astype(np.float32).astype(np.float64)
    if kind == "f64":
        vs = vs + rs.uniform(1e-10, 1e-9, vs.shape)
    z = np.sort(rs.uniform(0, 60, (N, ML)), axis=1)
    cols = np.arange(2 * ML)[None, :]
    nn = n[:, None]
    rows = np.where(cols < nn, np.take_along_axis(vs, np.minimum(cols, ML - 1), 1),
                    np.where(cols < 2 * nn, np.take_along_axis(z, np.clip(cols - nn, 0, ML - 1), 1), np.nan))
    return rows.astype(np.float32) if kind == "f32" else rows


def grid(D):
    return np.array([20.0]) if D == 1 else np.linspace(0, 70, D)


def loaded(models, site=None, engine=None, nsites=None):
    from bayhunter_amd.posterior import _Loaded
    return _Loaded(models, site, engine, nsites)


def raw(ld, dep, rank, R=None, D=None):
    """bh_posterior_column_quantiles with prefilled outputs: (rc, lower, upper, keys32)"""
    dep = np.ascontiguousarray(dep, np.float64)
    rank = np.ascontiguousarray(rank, np.uint32)
    shape = (ld.S, max(dep.size, 1), max(rank.shape[1], 1))
    lo, up = np.full(shape, FILL, np.uint64), np.full(shape, FILL, np.uint64)
    k32 = np.full(1, -7, np.int32)
    rc = ld._L.bh_posterior_column_quantiles(ld._p, dep.size if D is None else D, ptr(dep), rank.shape[1] if R is None else R,
                                             ptr(rank), ptr(lo), ptr(up), ptr(k32))
    return rc, lo, up, int(k32[0])


def want_keys(vsi, ranks, k32):
    """the keys of the order statistics ranks and ranks + 1 of every column of vsi [n, D]: [D, R] each"""
    s = np.sort(vsi, axis=0)
    n = len(s)
    ranks = np.asarray(ranks, np.int64)
    return okeys(s[ranks].T, k32), okeys(s[np.minimum(ranks + 1, n - 1)].T, k32)


# ---- bits against numpy -------------------------------------------------------------------------------------------------
# every number of rows (both sides of POST_CHUNK = 8192), depth count (inactive lanes, a second blockIdx.y), row width, kind of
# rows and quantile list occurs with 32-bit keys (f32, f64of32: 4 passes) and with 64-bit keys (f64: 8 passes)
CASES = [(1, 1, 2, "f32", "q2"), (2, 63, 6, "f64of32", "q1"), (3, 64, 32, "f32", "q5"), (8191, 65, 6, "f64of32", "q8"),
         (8192, 130, 2, "f32", "q9"), (8193, 64, 32, "f64of32", "qdup"), (16500, 65, 6, "f32", "q17"), (3, 130, 2, "f32", "quns"),
         (1, 63, 32, "f64", "q5"), (2, 1, 6, "f64", "q8"), (3, 65, 2, "f64", "q1"), (8191, 64, 2, "f64", "q2"),
         (8192, 63, 6, "f64", "quns"), (8193, 130, 6, "f64", "q9"), (16500, 64, 32, "f64", "q17"), (8193, 1, 2, "f64", "qdup")]


@pytest.mark.parametrize("N,D,ML,kind,ql", CASES, ids=["%d-%d-%d-%s-%s" % c for c in CASES])
def test_quantiles_are_numpys_bit_for_bit(N, D, ML, kind, ql, engine):
    from bayhunter_amd.posterior import column_quantiles, posterior_models
    rs = np.random.RandomState(N + D + ML)
    m, dep, q = synth(rs, N, ML, kind), grid(D), QLISTS[ql]
    want = np.quantile(R.interp(m, dep), q, axis=0, method="linear")
    ld = loaded(m, engine=engine)
    try:
        got = column_quantiles(ld, dep, q)
        _, _, _, k32 = raw(ld, dep, np.zeros((1, 1), np.uint32))
    finally:
        ld.close()
    assert k32 == (0 if kind == "f64" else 1)
    assert got.shape == (1, len(q), D) and bits_equal(got[0], want)
    if D >= 2:                                                   # (the summaries need two depths: their mode is per depth bin)
        r = posterior_models(m, dep_int=dep, quantiles=q, engine=engine)
        assert bits_equal(r["quantiles"][0], want) and np.array_equal(r["quantiles"][1], dep)
        assert r["q"].dtype == np.float64 and np.array_equal(r["q"], np.array(q))


# ---- ties, ranks that part in the last pass, the median -----------------------------------------------------------------

@pytest.mark.parametrize("kind", ("f32", "f64"))
def test_ranks_inside_and_at_the_ends_of_runs_of_ties(kind, engine):
    rs = np.random.RandomState(41)
    n, dep = 9000, grid(65)
    m = synth(rs, n, 6, "f32", ties=True)
    if kind == "f64":                                           # the same runs on 64-bit keys: one vs value that is not float32-exact
        m = m.astype(np.float64)
        m[0, 0] = 2.0 + 1e-12
    vsi = R.interp(m, dep)
    s = np.sort(vsi[:, 10])
    first = np.flatnonzero(np.diff(s) > 0) + 1                  # the first index of every run but the first
    i0, i1 = int(first[3]), int(first[4]) - 1
    assert i1 - i0 >= 2 and s[i0] == s[i1] and s[i0 - 1] < s[i0] < s[i1 + 1]
    ranks = [i0, i0 + 1, i1, i1 + 1, i0 - 1, 0, n - 1, (n - 1) // 2]
    ld = loaded(m, engine=engine)
    try:
        rc, lo, up, k32 = raw(ld, dep, np.array([ranks], np.uint32))
    finally:
        ld.close()
    assert rc == 0 and k32 == (kind == "f32")
    wl, wu = want_keys(vsi, ranks, kind == "f32")
    assert np.array_equal(lo[0], wl) and np.array_equal(up[0], wu)
    j = 10                                                      # inside the run and at its first element the next key is the same one,
    assert lo[0, j, 0] == up[0, j, 0] == lo[0, j, 1] == up[0, j, 1] == lo[0, j, 2] < up[0, j, 2] == lo[0, j, 3]   # at its last the next run's
    assert lo[0, j, 6] == up[0, j, 6]                           # (the last rank: upper == lower)


@pytest.mark.parametrize("kind", ("f32", "f64"))
def test_two_ranks_that_share_counters_until_the_last_pass(kind, engine):
    """keys that differ in the lowest digit only: 3.0 and the next number above it"""
    T = np.float32 if kind == "f32" else np.float64
    a = T(3.0)
    b = np.nextafter(a, T(4.0))
    vs = np.concatenate((np.full(5, 2.0), np.full(40, a), np.full(40, b), np.full(5, 4.0))).astype(T)
    m = np.full((90, 4), np.nan, T)
    m[:, 0], m[:, 1] = vs, 0.0                                  # one-layer rows: every column is vs itself
    m = m[np.random.RandomState(2).permutation(90)]
    ranks = [10, 44, 45, 84, 0, 89]
    ld = loaded(m, engine=engine)
    try:
        rc, lo, up, k32 = raw(ld, np.array([1.0, 2.0]), np.array([ranks], np.uint32))
    finally:
        ld.close()
    assert rc == 0 and k32 == (kind == "f32")
    ka, kb = int(okeys(a, k32 == 1)), int(okeys(b, k32 == 1))
    assert kb == ka + 1 and (ka >> 8) == (kb >> 8)
    k2, k4 = int(okeys(T(2.0), k32 == 1)), int(okeys(T(4.0), k32 == 1))
    for j in range(2):
        assert [int(v) for v in lo[0, j]] == [ka, ka, kb, kb, k2, k4]
        assert [int(v) for v in up[0, j]] == [ka, kb, kb, k4, k2, k4]


@pytest.mark.parametrize("n", (8200, 8201, 2, 1))
def test_the_middle_ranks_are_the_medians_keys(n, engine):
    rs = np.random.RandomState(n)
    for kind in ("f32", "f64"):
        m, dep = synth(rs, n, 6, kind, ties=(kind == "f32")), grid(65)
        ld = loaded(m, engine=engine)
        try:
            col = ld.columns(dep, median=True)
            rc, lo, up, k32 = raw(ld, dep, np.array([[(n - 1) // 2]], np.uint32))
        finally:
            ld.close()
        assert rc == 0 and bool(k32) == col["keys32"]
        assert np.array_equal(lo[0, :, 0], col["median"][0, :, 0]) and np.array_equal(up[0, :, 0], col["median"][0, :, 1])


def test_two_ranks_on_both_layouts_beside_an_empty_and_a_one_row_site(engine):
    """R = 2, the smallest call that takes the select's wide instantiation, over the depth columns and over a scalar set (a
    float32-exact column and a float64 column with NaNs: both key widths in one call) of a site of 8193 rows (two chunks), an
    empty site and a one-row site: numpy.sort's keys bit for bit, and the keys of the R = 1 calls of the same ranks"""
    from bayhunter_amd import engine as E
    from bayhunter_amd.posterior import _Loaded
    rs = np.random.RandomState(8193)
    counts = (8193, 0, 1)
    m, dep = synth(rs, sum(counts), 6, "f32"), grid(65)
    site = np.concatenate([np.full(n, s, np.int32) for s, n in enumerate(counts)])[rs.permutation(sum(counts))]
    u = np.stack((rs.normal(0, 1, len(m)).astype(np.float32).astype(np.float64), rs.normal(5, 2, len(m)) + 1e-10), axis=1)
    u[rs.randint(0, len(m), 300), 1] = np.nan
    u[site == 2, 1] = np.nan                                    # the one-row site: a column without a value
    crank = np.array([[17, 8192], [0, 0], [0, 0]], np.uint32)
    ld = _Loaded(m, site, engine, 3, scalars=True)
    try:
        rc, lo, up, k32 = raw(ld, dep, crank)
        ones = [raw(ld, dep, crank[:, r:r + 1]) for r in range(2)]
        ld.attach(u, False)
        cnt = ld.scalar_stats(E.SCALARS_USER)["count"]
        srank = np.stack((cnt // 3, np.maximum(cnt - 1, 0)), axis=2).astype(np.uint32)
        slo, sup = ld.quantile_keys(E.SCALARS_USER, srank)
        sones = [ld.quantile_keys(E.SCALARS_USER, srank[:, :, r:r + 1]) for r in range(2)]
    finally:
        ld.close()
    assert rc == 0 and k32 == 1
    assert cnt[0, 0] == 8193 and 7800 < cnt[0, 1] < 8193 and not cnt[1].any() and [int(c) for c in cnt[2]] == [1, 0]
    for s in range(3):
        if not counts[s]:
            assert not lo[s].any() and not up[s].any()
            continue
        wl, wu = want_keys(R.interp(m[site == s], dep), crank[s], True)
        assert np.array_equal(lo[s], wl) and np.array_equal(up[s], wu), s
    for s in range(3):
        for q in range(2):
            v = np.sort(u[site == s, q][~np.isnan(u[site == s, q])])
            if not len(v):
                assert not slo[s, q].any() and not sup[s, q].any()
                continue
            k = srank[s, q].astype(np.int64)
            assert np.array_equal(slo[s, q], okeys(v[k], False)) and np.array_equal(sup[s, q], okeys(v[np.minimum(k + 1, len(v) - 1)], False)), (s, q)
    for r in range(2):
        assert ones[r][0] == 0 and np.array_equal(ones[r][1][:, :, 0], lo[:, :, r]) and np.array_equal(ones[r][2][:, :, 0], up[:, :, r])
        assert np.array_equal(sones[r][0][:, :, 0], slo[:, :, r]) and np.array_equal(sones[r][1][:, :, 0], sup[:, :, r])


# ---- independence -------------------------------------------------------------------------------------------------------

def test_sites_among_others_alone_again_and_from_device_rows(engine):
    import torch
    from bayhunter_amd.posterior import posterior_models
    rs = np.random.RandomState(8)
    dep = grid(70)
    for kind in ("f32", "f64"):
        per = [synth(rs, 8300, 6, kind), synth(rs, 0, 6, kind), synth(rs, 1, 6, kind), synth(rs, 300, 6, kind, ties=True)]
        rows = np.concatenate(per)
        site = np.concatenate([np.full(len(p), s, np.int32) for s, p in enumerate(per)])
        perm = rs.permutation(len(rows))
        a = posterior_models(rows[perm], site=site[perm], dep_int=dep, quantiles=QLISTS["q9"], engine=engine, nsites=4)
        b = posterior_models(rows[perm], site=site[perm], dep_int=dep, quantiles=QLISTS["q9"], engine=engine, nsites=4)
        same(a, b)
        assert a[1]["count"] == 0 and np.all(np.isnan(a[1]["quantiles"][0])) and a[1]["quantiles"][0].shape == (9, 70)
        for s in (0, 2, 3):
            alone = posterior_models(per[s], dep_int=dep, quantiles=QLISTS["q9"], engine=engine)
            same(alone, a[s], (kind, s))
            assert bits_equal(a[s]["quantiles"][0], np.quantile(R.interp(per[s], dep), QLISTS["q9"], axis=0, method="linear"))
        # device rows, rows that are no samples (site -1) among them: dropped
        extra = synth(rs, 500, 6, kind)
        mixed = np.concatenate((rows, extra))[np.concatenate((perm, len(rows) + np.arange(500)))]
        msite = np.concatenate((site[perm], np.full(500, -1, np.int32)))
        again = rs.permutation(len(mixed))
        d = posterior_models(torch.from_numpy(mixed[again]).cuda(), site=torch.from_numpy(msite[again]).cuda(), dep_int=dep,
                             quantiles=QLISTS["q9"], engine=engine, nsites=4)
        same(d, a, (kind, "device"))


# ---- the golden sets ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", KEYS)
def test_golden_sets_gain_their_quantiles_and_nothing_else_moves(G, key, engine):
    from bayhunter_amd.posterior import posterior_models
    m, dep = G[key + "_models"], G["dep_int"]
    q = QLISTS["q17"]
    r = posterior_models(m, dep_int=dep, misfits=G[key + "_misfits"], quantiles=q, engine=engine)
    assert bits_equal(r["quantiles"][0], np.quantile(R.interp(m, dep), q, axis=0, method="linear"))
    assert np.array_equal(r["quantiles"][1], dep) and np.array_equal(r["q"], np.array(q))
    plain = posterior_models(m, dep_int=dep, misfits=G[key + "_misfits"], engine=engine)
    assert set(plain) == MODEL_KEYS | {"minmisfit"} and set(r) == set(plain) | {"quantiles", "q"}
    same({k: r[k] for k in plain}, plain)
    # the order statistics behind quantile 0.5 and the median are the same keys: equal for an odd count, within an ulp else
    half = r["quantiles"][0][8]
    assert np.all(np.abs(half - r["median"][0]) <= np.spacing(r["median"][0]))


# ---- Moho and scalar columns ----------------------------------------------------------------------------------------------

def column_quantile(v, q):
    v = np.asarray(v, np.float64)
    v = v[~np.isnan(v)]
    return np.quantile(v, q, method="linear") if v.size else np.full(len(q), np.nan)


def test_moho_and_scalar_columns_with_quantiles(engine):
    from bayhunter_amd import posterior_moho, posterior_scalars
    from test_gpu_posterior_scalars import crust_rows
    rs = np.random.RandomState(77)
    per = [crust_rows(rs, 8300), crust_rows(rs, 41).astype(np.float64), crust_rows(rs, 60)]
    per[2][:, 0] = 2.0
    per[2][:, 1:12] = np.minimum(per[2][:, 1:12], 3.0)                    # a site where no row has a Moho
    rows = np.concatenate([p.astype(np.float64) for p in per])
    site = np.concatenate([np.full(len(p), s, np.int32) for s, p in enumerate(per)])
    lo, hi, mv = [3.0, 0.0, 5.0], [45.0, 50.0, 40.0], [4.1, 4.0, 4.2]
    q = QLISTS["q9"]
    a = posterior_moho(rows, site=site, moho=np.stack((lo, hi), 1), mohovs=mv, quantiles=q, engine=engine)
    plain = posterior_moho(rows, site=site, moho=np.stack((lo, hi), 1), mohovs=mv, engine=engine)
    assert a[0]["count"] > 3000 and a[2]["count"] == 0
    for s in range(3):
        v = MR.moho_rows(per[s].astype(np.float64), lo[s], hi[s], mv[s])
        for i, name in enumerate(MR.COLUMNS):
            assert set(plain[s][name]) == STAT_KEYS and set(a[s][name]) == STAT_KEYS | {"quantiles"}
            assert a[s][name]["quantiles"].dtype == np.float64 and bits_equal(a[s][name]["quantiles"], column_quantile(v[:, i], q)), (s, name)
            a[s][name].pop("quantiles")
        same(a[s], plain[s], (s,))
    assert np.all(np.isnan(plain[2]["moho"]["median"]))
    # scalar columns: a float32 one, one with NaNs, a constant one, a [N, 2] one, and nlayers
    N = len(rows)
    f32 = rs.normal(0, 1, N).astype(np.float32)
    holes = rs.normal(5, 2, N)
    holes[rs.randint(0, N, 400)] = np.nan
    holes[site == 2] = np.nan                                            # ... and a site where the column has no value at all
    const = np.full(N, 1.75)
    pair = rs.uniform(0, 1, (N, 2))
    cols = dict(f32=f32, holes=holes, const=const, pair=pair)
    c = posterior_scalars(rows, cols, site=site, quantiles=Q5, engine=engine)
    cp = posterior_scalars(rows, cols, site=site, engine=engine)
    for s in range(3):
        mine = site == s
        wants = dict(f32=f32[mine].astype(np.float64), holes=holes[mine], const=const[mine], nlayers=MR.nlayers(rows[mine]))
        for name, v in wants.items():
            assert set(cp[s][name]) == SCALAR_KEYS and set(c[s][name]) == SCALAR_KEYS | {"quantiles"}
            assert c[s][name]["quantiles"].dtype == np.float64 and bits_equal(c[s][name]["quantiles"], column_quantile(v, Q5)), (s, name)
        for i in range(2):
            assert bits_equal(c[s]["pair"][i]["quantiles"], column_quantile(pair[mine, i], Q5))
        assert np.all(c[s]["const"]["quantiles"] == 1.75) and c[s]["const"]["constant"]
        for name in list(wants) + ["pair"]:
            for d in (c[s][name] if name == "pair" else [c[s][name]]):
                d.pop("quantiles")
        same(c[s], cp[s], (s,))
    assert c[2]["holes"]["count"] == 0 and np.all(np.isnan(column_quantile(holes[site == 2], Q5)))


def test_without_quantiles_the_results_have_todays_keys(engine):
    from bayhunter_amd import posterior_models, posterior_moho, posterior_scalars
    m = synth(np.random.RandomState(1), 50, 6, "f32")
    assert set(posterior_models(m, engine=engine)) == MODEL_KEYS
    r = posterior_moho(m, moho=(5.0, 40.0), engine=engine)
    assert set(r) == {"rows", "count", "invalid_rows", "dropped", "hist", "hist2d", "mode"} | set(MR.COLUMNS)
    assert all(set(r[k]) == STAT_KEYS for k in MR.COLUMNS)
    c = posterior_scalars(m, dict(v=np.arange(50.0)), engine=engine)
    assert set(c) == {"rows", "invalid_rows", "dropped", "v", "nlayers"} and set(c["v"]) == set(c["nlayers"]) == SCALAR_KEYS
    e = posterior_models(m, quantiles=(), engine=engine)                  # an empty list: the keys, no values
    assert e["quantiles"][0].shape == (0, 201) and e["q"].shape == (0,)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------

def test_header_symbols_and_refusals_that_write_nothing(engine):
    import os
    import re
    from bayhunter_amd import engine as E
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(here, "include", "bh_engine_posterior_quantiles.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(bh_[a-z_0-9]+)\s*\(", txt))) == sorted(E.POSTERIOR_QUANTILES_SYMBOLS)
    lib = E.load_library()
    assert all(hasattr(lib, n) for n in E.POSTERIOR_QUANTILES_SYMBOLS) and lib.bh_abi_version() == 10
    rs = np.random.RandomState(3)
    rows = np.concatenate((synth(rs, 30, 6, "f32"), synth(rs, 20, 6, "f32")))
    site = np.concatenate((np.zeros(30, np.int32), np.full(20, 2, np.int32)))          # site 1 has no rows
    dep = grid(5)
    ld = loaded(rows, site, engine=engine, nsites=3)
    try:
        def refused(res, text):
            rc, lo, up, k32 = res
            assert rc == E.BH_EINVAL and np.all(lo == FILL) and np.all(up == FILL) and k32 == -7
            with pytest.raises(E.EngineError, match=text):
                engine._check(rc)

        ok = np.array([[29, 0], [0, 0], [19, 7]], np.uint32)
        refused(raw(ld, dep, ok, R=0), "BH_QUANTILES_MAXRANKS")
        refused(raw(ld, dep, np.zeros((3, 9), np.uint32)), "BH_QUANTILES_MAXRANKS")
        for s, n in ((0, 30), (1, 1), (2, 20)):                                         # a rank equal to the site's count (1 for
            bad = ok.copy()                                                             # the site without rows)
            bad[s, 1] = n
            refused(raw(ld, dep, bad), "rank")
        refused(raw(ld, np.array([0.0, 10.0, 10.0, 20.0, 30.0]), ok), "ascending")
        refused(raw(ld, np.array([0.0, 10.0, np.inf, 20.0, 30.0]), ok), "ascending")
        refused(raw(ld, dep, ok, D=0), "depth grid")
        rc, lo, up, k32 = raw(ld, dep, ok)                                              # ... and the call they refuse
        assert rc == 0 and k32 == 1 and np.all(lo[1] == 0) and np.all(up[1] == 0) and np.all(lo[0] != FILL)
        wl, wu = want_keys(R.interp(rows[30:], dep), ok[2], True)
        assert np.array_equal(lo[2], wl) and np.array_equal(up[2], wu)
        # a handle that has loaded nothing
        h = C.c_void_p()
        engine._check(lib.bh_posterior_create(engine._h, C.byref(h)))
        try:
            fresh = type("H", (), dict(_L=lib, _p=h, S=3))()
            refused(raw(fresh, dep, ok), "no rows loaded")
        finally:
            lib.bh_posterior_destroy(h)
    finally:
        ld.close()


# ---- chains ---------------------------------------------------------------------------------------------------------------

DEP = np.linspace(0, 80, 33)


def test_chains_summarise_their_device_record_with_quantiles(tmp_path, engine):
    """2 sites x 4 chains under their own priors: the summaries from the device store equal the free functions on the host arrays of
    samples(site=s); exclude_chains is honoured; the saved folders give the same numbers"""
    import bayhunter_amd as bh
    from bayhunter_amd.device_chains import DeviceChains
    from test_gpu_posterior_scalars import chain_columns, site_targets
    from test_gpu_sites_priors import SITE_INIT, SITE_PRIORS
    T, Cn = 100, 4
    inits = [dict(SITE_INIT[s], iter_burnin=100, iter_main=T, maxmodels=T, savepath=str(tmp_path)) for s in range(2)]
    dc = DeviceChains(site_targets(), Cn, inits, SITE_PRIORS[:2], seed=78, search="fast", record="device").run()
    assert dc.thinning == 1 and dc.nsamples("p2") == T
    mv = [3.6, 3.8]
    pm = dc.posterior_models(dep_int=DEP, quantiles=Q5)
    ph = dc.posterior_hist2d()
    pmo = dc.posterior_moho(mohovs=mv, quantiles=Q5)
    ps = dc.posterior_scalars(quantiles=Q5)
    ex = dc.posterior_models(dep_int=DEP, quantiles=Q5, exclude_chains=(1, 6))
    assert "quantiles" not in dc.posterior_models(dep_int=DEP)[0] and "quantiles" not in dc.posterior_moho(mohovs=mv)[0]["moho"]
    n = T * Cn
    hosts = []
    for s in range(2):
        h = dc.samples("p2", site=s)
        m = h["models"].reshape(n, -1)
        mis = h["misfits"][..., -1].reshape(n)
        hosts.append((m, mis))
        want = bh.posterior_models(m, dep_int=DEP, misfits=mis, quantiles=Q5, engine=engine)
        assert "minmisfit" in pm[s] and pm[s]["count"] == n
        same(pm[s], want, (s, "models"))
        assert bits_equal(pm[s]["quantiles"][0], np.quantile(R.interp(m, DEP), Q5, axis=0, method="linear"))
        same(ph[s], bh.posterior_hist2d(m, engine=engine), (s, "hist2d"))
        same(pmo[s], bh.posterior_moho(m, moho=SITE_PRIORS[s]["z"], mohovs=mv[s], quantiles=Q5, engine=engine), (s, "moho"))
        same(ps[s], bh.posterior_scalars(m, chain_columns(h, n), quantiles=Q5, engine=engine), (s, "scalars"))
        keep = np.ones(Cn, bool)
        keep[[1] if s == 0 else [2]] = False                               # chains 1 | 6
        mk = h["models"][:, keep].reshape(T * 3, -1)
        wk = bh.posterior_models(mk, dep_int=DEP, misfits=h["misfits"][..., -1][:, keep].reshape(T * 3), quantiles=Q5, engine=engine)
        assert ex[s]["count"] == T * 3
        same(ex[s], wk, (s, "excluded"))
    # the saved folders (no chain is an outlier at dev = 10): the readers pass quantiles on
    paths = dc.save(str(tmp_path))
    for p in paths:
        bh.save_final_distribution(p, maxmodels=10 * n, dev=10.0)
    fm = bh.posterior_from_storage(paths, dep_int=DEP, quantiles=Q5, engine=engine)
    fo = bh.moho_from_storage(paths, mohovs=mv, quantiles=Q5, engine=engine)
    assert "quantiles" not in bh.posterior_from_storage(paths, dep_int=DEP, engine=engine)[0]
    assert "quantiles" not in bh.moho_from_storage(paths, mohovs=mv, engine=engine)[0]["moho"]
    for s in range(2):
        cm = np.load(paths[s] + "/c_models.npy")
        assert len(cm) == n and fm[s]["count"] == n and fo[s]["rows"] == n
        assert bits_equal(fm[s]["quantiles"][0], np.quantile(R.interp(cm, DEP), Q5, axis=0, method="linear"))
        same(fo[s], bh.posterior_moho(cm, moho=SITE_PRIORS[s]["z"], mohovs=mv[s], quantiles=Q5, engine=engine), (s, "stored moho"))
        # the files hold float64 copies of the device's float32 rows: the vs values, and with them the order statistics of vs, are
        # the device's (an interface depth is a float64 mean there and a float32 one on the device: the Moho DEPTH may differ in
        # its last bits, the vs of the last crustal layer may not)
        assert bits_equal(fm[s]["quantiles"][0], pm[s]["quantiles"][0])
        assert bits_equal(fo[s]["vslast"]["quantiles"], pmo[s]["vslast"]["quantiles"])


def test_tempered_chains_take_their_cold_rows(engine):
    """one ladder of 4 temperatures per site: the beta = 1 rows are selected on the device"""
    import bayhunter_amd as bh
    from bayhunter_amd.device_chains import DeviceChains
    from test_gpu_chains import SETUPS
    from test_gpu_posterior_scalars import chain_columns, site_targets
    su = SETUPS["exp"]
    T = 80
    init = dict(su["init"], iter_burnin=160, iter_main=T, maxmodels=T)
    ladder = np.repeat(np.arange(2), 4)
    betas = np.tile(1.0 / np.geomspace(1.0, 20.0, 4), 2)
    dc = DeviceChains(site_targets(), 4, init, su["priors"], seed=6, betas=betas, ladder=ladder, swap_every=20,
                      record="device").run()
    pm, ph = dc.posterior_models(dep_int=DEP, quantiles=Q5), dc.posterior_hist2d()          # cold_only by default
    pmo, ps = dc.posterior_moho(mohovs=3.7, quantiles=Q5), dc.posterior_scalars(quantiles=Q5)
    every = dc.posterior_models(dep_int=DEP, quantiles=Q5, cold_only=False)
    for s in range(2):
        h = dc.samples("p2", cold_only=True, site=s)
        assert h["models"].shape[:2] == (T, 1) and np.all(h["beta"] == 1.0)
        m = h["models"].reshape(T, -1)
        assert pm[s]["count"] == ph[s]["count"] == T and every[s]["count"] == 4 * T
        same(pm[s], bh.posterior_models(m, dep_int=DEP, misfits=h["misfits"][..., -1].reshape(T), quantiles=Q5, engine=engine), (s, "models"))
        same(ph[s], bh.posterior_hist2d(m, engine=engine), (s, "hist2d"))
        want, wc = bh.posterior_moho(m, moho=su["priors"]["z"], mohovs=3.7, quantiles=Q5, engine=engine), \
            bh.posterior_scalars(m, chain_columns(h, T), quantiles=Q5, engine=engine)
        for x in (pmo[s], ps[s], want, wc):
            x.pop("dropped")
        same(pmo[s], want, (s, "moho"))
        same(ps[s], wc, (s, "scalars"))
