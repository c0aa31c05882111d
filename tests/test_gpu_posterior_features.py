"""Structural features of the layered models as a scalar set on the GPU (include/bh_engine_posterior_features.h,
bayhunter_amd/posterior.py: posterior_features) against the restatement tests/features_ref.py, which tests/test_features_ref.py
holds to the step model's integrals, the Moho rule and numpy: the feature table bit for bit, NaN where and only where the
restatement has NaN; then the passes behind the set, the covariance, the refusals and the callers."""
import ctypes as C

import numpy as np
import pytest

import features_ref as FR
from test_features_ref import row_of
from test_gpu_posterior_quantiles import same

pytestmark = pytest.mark.gpu

# one feature of every kind, in the order of BH_FEATURE_*; 13 columns
KINDS = list(FR.KINDS)
COLS = ["vsmean", "vstime", "tts", "vsmin.value", "vsmin.depth", "vsmax.value", "vsmax.depth", "drop.depth", "drop.jump",
        "jump.depth", "jump.jump", "above", "nifaces"]
OPTIONAL = dict(drop=7, jump=9, above=11)        # the first column of the kinds a row may lack
S4 = 4                                           # four sites with their own windows and thresholds; site 2 has no rows


def site_par(family, ML):
    """[4][9][3]: every site's (z0, z1, c) of the nine kinds -- on the grid of 0.25 km for the rows of family "a".  The thresholds
    were chosen on the CPU (features_ref alone) so that every optional feature is there in at least a tenth of every populated
    site's rows and missing in at least a tenth: test_the_feature_table_is_the_restatements asserts it."""
    par = np.zeros((S4, 9, 3))
    win = [(5.0, 30.0), (0.0, 45.25), (2.0, 9.0), (12.5, 50.0)]
    if family == "a":
        drop = [1.0, 1.5, 0.5, 1.25] if ML == 4 else [2.5, 3.0, 1.0, 2.75]
        jump = [0.75, 1.5, 0.5, 1.0] if ML == 4 else [2.75, 3.0, 1.0, 2.5]
        above = [3.5, 3.0, 3.0, 4.0] if ML == 4 else [4.75, 4.5, 4.0, 4.75]
    else:
        drop = [0.5, 0.75, 0.5, 0.4] if ML == 4 else [1.9, 2.1, 1.0, 1.8]
        jump = [0.4, 0.8, 0.5, 0.5] if ML == 4 else [1.8, 2.2, 1.0, 1.9]
        above = [3.4, 3.2, 3.0, 3.6] if ML == 4 else [4.6, 4.7, 4.0, 4.65]
    for s in range(S4):
        par[s, :, 0], par[s, :, 1] = win[s]
        par[s, 2, :2] = (0.0, 3.0 + s)                              # tts from the surface
        par[s, 3, :2] = (win[s][0] + 1.0, win[s][1] + 10.0)         # vsmin and the others in windows of their own
        par[s, 8, :2] = (0.25 * s, 20.0 + 5 * s)
        par[s, 5, 2], par[s, 6, 2], par[s, 7, 2] = drop[s], jump[s], above[s]
    return par


def make_rows(rs, N, ML, dtype, family):
    """N rows with n = 1..ML layers in turn (a half-space alone has no interface, n = ML no NaN padding).
    family "a": interface depths on the grid of 0.25 km in [0, 55] -- many on a window edge, some equal (layers of no thickness),
    some 0 -- and vs on the grid of 0.25 km/s (equal velocities, equal jumps); "b": continuous z in [0, 60] and vs in [2, 4.8]"""
    rows = np.full((N, 2 * ML), np.nan)
    n_all = 1 + (np.arange(N) + rs.randint(ML)) % ML
    for i, n in enumerate(n_all):
        if family == "a":
            dep = np.sort(rs.randint(0, 221, n - 1)) * 0.25
            if n > 2 and i % 5 == 0:
                dep[1] = dep[0]
            rows[i] = row_of(rs.randint(6, 21, n) * 0.25, dep, np.float64, ML)
        else:
            rows[i, :n], rows[i, n:2 * n] = rs.uniform(2.0, 4.8, n), np.sort(rs.uniform(0, 60, n))
    return rows.astype(dtype)


def special_rows(ML, dtype, z0, z1):
    """two rows for a site whose windows lie in [z0 + 0.25, z1]: every such window wholly inside one layer, and wholly inside the
    half-space"""
    a = row_of([2.0, 3.25, 4.5], [0.25, z1 + 1.0], dtype, ML)
    b = row_of([2.5, 3.75], [0.25], dtype, ML)
    return np.array([a, b])


_CASES = {}


def case(ML, dtype, N, family):
    """(rows, site, par, reference table [13][N]) of one case, built once"""
    key = (ML, np.dtype(dtype).str, N, family)
    if key not in _CASES:
        rs = np.random.RandomState(1000 + 7 * ML + N + (family == "b"))
        rows = make_rows(rs, N, ML, dtype, family)
        par = site_par(family, ML)
        if N == 1:
            site = np.array([1], np.int32)
        elif N > 8192:
            site = np.full(N, 1, np.int32)                     # one site: two work items of it in the passes behind
        else:
            site = rs.choice(np.array([0, 1, 3], np.int32), N)
            where = np.flatnonzero(site == 0)[:2]
            rows[where] = special_rows(ML, dtype, 0.0, 45.0)   # site 0's windows all lie inside [0.25, 46]
        if N > 1 and ML >= 3:
            assert np.isnan(rows).all(0).sum() == 0            # some row has n = ML
        ref = FR.features_ref(rows, KINDS, par, site)
        _CASES[key] = (rows, site, par, ref)
    return _CASES[key]


def fractions(ref, site):
    """{(kind, site): the part of the site's rows that have the optional feature}"""
    return {(k, s): float(np.mean(~np.isnan(ref[c, site == s]))) for k, c in OPTIONAL.items() for s in np.unique(site)}


def loaded(models, site, engine, nsites, scalars=True):
    from bayhunter_amd.posterior import _Loaded
    return _Loaded(models, site, engine, nsites, scalars=scalars)


def gathered(ld, which, ninput, Q):
    """([Q][ninput] the set's table in the order of the input rows, NaN in the columns of rows the load left out; kept [ninput])
    -- the input index of every loaded row comes back through a USER column"""
    from bayhunter_amd import engine as E
    ld.attach(np.arange(ninput, dtype=np.float64)[:, None], False)
    order = ld.gather(E.SCALARS_USER, np.arange(int(ld.rows.sum())), 1)[:, 0].astype(np.int64)
    g = ld.gather(which, np.arange(int(ld.rows.sum())), Q)
    out = np.full((g.shape[1], ninput), np.nan)
    out[:, order] = g.T
    kept = np.zeros(ninput, bool)
    kept[order] = True
    assert kept.sum() == len(order)
    return out, kept


CASES = [(4, np.float32, 1, "a"), (32, np.float64, 1, "b"),
         (4, np.float64, 255, "b"), (32, np.float32, 255, "a"),
         (4, np.float32, 257, "b"), (4, np.float64, 257, "a"), (32, np.float32, 257, "b"), (32, np.float64, 257, "a"),
         (4, np.float32, 8193, "a"), (4, np.float64, 8193, "b")]


@pytest.mark.parametrize("memspace", ["host", "device"])
@pytest.mark.parametrize("ML, dtype, N, family", CASES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_the_feature_table_is_the_restatements(ML, dtype, N, family, memspace, engine):
    from bayhunter_amd import engine as E
    rows, site, par, ref = case(ML, dtype, N, family)
    if N > 1:        # no vacuous pass: every optional feature is there and missing in a tenth of every populated site's rows
        fr = fractions(ref, site)
        assert all(0.1 <= v <= 0.9 for v in fr.values()), fr
        assert not np.isnan(ref[[0, 1, 2, 3, 4, 5, 6, 12]]).any()
    m, st, ninput = rows, site, N
    if memspace == "device":
        import torch
        extra = np.repeat(rows[:1], 3, axis=0)                             # rows of site -1: dropped and counted
        m = torch.from_numpy(np.concatenate((rows[:N // 2], extra, rows[N // 2:]))).cuda()
        st = torch.from_numpy(np.concatenate((site[:N // 2], np.full(3, -1, np.int32), site[N // 2:]))).cuda()
        ninput = N + 3
    ld = loaded(m, st, engine, S4)
    try:
        assert ld.dropped == (3 if memspace == "device" else 0) and ld.rows.sum() == N and ld.rows[2] == 0
        found = ld.features(np.arange(9), par)
        t, kept = gathered(ld, E.SCALARS_FEATURES, ninput, 13)
        stats = ld.scalar_stats(E.SCALARS_FEATURES) if N > 8192 else None
    finally:
        ld.close()
    if memspace == "device":
        assert not kept[N // 2:N // 2 + 3].any()
        t = np.delete(t, np.arange(N // 2, N // 2 + 3), axis=1)
    assert t.shape == ref.shape == (13, N)
    bad = [(COLS[c], r) for c, r in zip(*np.nonzero(~((t == ref) | (np.isnan(t) & np.isnan(ref)))))]
    assert not bad, bad[:10]
    assert np.array_equal(t, ref, equal_nan=True)
    want = np.array([[np.sum(~np.isnan(ref[c, site == s])) for c in range(13)] for s in range(S4)])
    assert np.array_equal(found, want)
    if stats is not None:
        assert np.array_equal(stats["count"], want) and np.array_equal(stats["nan"][1], N - want[1])
        assert np.array_equal(stats["min"][1], np.nanmin(ref, axis=1)) and np.array_equal(stats["max"][1], np.nanmax(ref, axis=1))


def test_above_with_the_mohos_parameters_is_the_moho_sets_depth(engine):
    from bayhunter_amd import engine as E
    rows, site, par, _ = case(32, np.float32, 257, "b")
    lo, hi, mv = np.array([5.0, 0.0, 1.0, 12.5]), np.array([30.0, 45.0, 2.0, 50.0]), np.array([4.5, 4.4, 4.0, 4.6])
    ld = loaded(rows, site, engine, S4)
    try:
        nm = ld.moho(lo, hi, mv)
        nf = ld.features([E.FEATURE_ABOVE], np.stack((lo, hi, mv), axis=1)[:, None, :])
        a, _ = gathered(ld, E.SCALARS_FEATURES, len(rows), 1)
        b, _ = gathered(ld, E.SCALARS_MOHO, len(rows), 4)
    finally:
        ld.close()
    assert np.array_equal(nm, nf[:, 0]) and 26 < nm.sum() < 231       # (with and without a Moho: a tenth of the rows each)
    assert a.shape == (1, 257) and np.array_equal(a[0], b[0], equal_nan=True)


def test_a_site_alone_among_others_permuted_and_again(engine):
    from bayhunter_amd import engine as E
    rows, site, par, ref = case(32, np.float64, 257, "a")
    rs = np.random.RandomState(8)

    def table(m, st, p, S):
        ld = loaded(m, st, engine, S)
        try:
            f = ld.features(np.arange(9), p)
            return gathered(ld, E.SCALARS_FEATURES, len(m), 13)[0], f
        finally:
            ld.close()

    t, f = table(rows, site, par, S4)
    t2, f2 = table(rows, site, par, S4)
    assert np.array_equal(t, t2, equal_nan=True) and np.array_equal(f, f2)             # again
    perm = rs.permutation(len(rows))
    tp, fp = table(rows[perm], site[perm], par, S4)
    assert np.array_equal(tp, t[:, perm], equal_nan=True) and np.array_equal(fp, f)    # the rows permuted
    for s in (0, 1, 3):
        sel = site == s
        ta, fa = table(rows[sel], None, par[s:s + 1], 1)                               # the site alone
        assert np.array_equal(ta, t[:, sel], equal_nan=True) and np.array_equal(fa[0], f[s])
    assert np.array_equal(t, ref, equal_nan=True)


# ---- the passes behind the set ---------------------------------------------------------------------------------------------

FEATURES = dict(upper=("vsmean", 0, 15), vs1k=("vstime", 0, [1.0, 1.5, 2.0]), sed_t=("tts", 0, 2.5), slow=("vsmin", 0, 60),
                fast=("vsmax", 5, [40, 50, 60]), lvz=("drop", 5, 60, [1.0, 1.2, 1.4]), step=("jump", [10, 15, 20], 55, 1.1),
                basement=("above", 0, 20, [3.3, 3.5, 3.7]), crustal=("nifaces", 0, 40))
LABELS = ["upper", "vs1k", "sed_t", "slow.value", "slow.depth", "fast.value", "fast.depth", "lvz.depth", "lvz.jump", "step.depth",
          "step.jump", "basement", "crustal"]
QS = (0.025, 0.5, 0.975, 1.0, 0.0, 0.3)


@pytest.fixture(scope="module")
def three_sites():
    """3 sites, 2 000 rows of up to 12 layers, float32, in any order; the reference table of FEATURES"""
    from bayhunter_amd.posterior import check_features
    rs = np.random.RandomState(77)
    rows = make_rows(rs, 2000, 12, np.float32, "b")
    site = rs.randint(0, 3, 2000).astype(np.int32)
    kinds, par, labels = check_features(FEATURES, 3)
    assert labels == LABELS
    return rows, site, FR.features_ref(rows, kinds, par, site)


def check_stats(d, v, bins, nifaces=False, quantiles=True):
    """a statistics dict of posterior_features against numpy on the reference column v (float64, NaN = no value)"""
    x = v[~np.isnan(v)]
    assert (d["count"], d["nan"]) == (len(x), len(v) - len(x)) and len(x) > 20
    assert (d["min"], d["max"], d["median"]) == (x.min(), x.max(), np.median(x))
    assert d["constant"] == bool(x.min() == x.max()) and not d["constant"]
    edges = np.arange(x.min(), x.max() + 2) - 0.5 if nifaces else np.histogram_bin_edges(x, bins)
    cnt = np.histogram(x, edges)[0]
    assert np.array_equal(d["hist"][1], edges) and np.array_equal(d["hist"][0], cnt) and d["hist"][0].sum() == len(x)
    assert d["mode"] == ((edges[:-1] + edges[1:]) / 2.)[np.argmax(cnt)]
    assert abs(d["mean"] - x.mean()) <= 1e-12 * abs(x.mean()) and abs(d["std"] - x.std()) <= 1e-10 * x.std()
    if quantiles:
        assert np.array_equal(d["quantiles"], np.quantile(x, QS, method="linear"))


def test_posterior_features_gives_numpys_statistics_of_the_reference_columns(three_sites, engine):
    import bayhunter_amd as bh
    rows, site, ref = three_sites
    bins = 30
    r = bh.posterior_features(rows, FEATURES, site=site, bins=bins, quantiles=QS, engine=engine)
    assert len(r) == 3
    for s in range(3):
        sel = site == s
        assert (r[s]["rows"], r[s]["invalid_rows"], r[s]["dropped"]) == (int(sel.sum()), 0, 0)
        assert sorted(r[s]) == sorted(list(FEATURES) + ["rows", "invalid_rows", "dropped"])
        col = {name: ref[c, sel] for c, name in enumerate(LABELS)}
        for name in ("upper", "vs1k", "sed_t", "basement"):
            check_stats(r[s][name], col[name], bins)
        check_stats(r[s]["crustal"], col["crustal"], bins, nifaces=True)
        for name, part in (("slow", "value"), ("fast", "value"), ("lvz", "jump"), ("step", "jump")):
            d = r[s][name]
            assert sorted(d) == sorted(["depth", part, "hist2d", "mode"] + (["probability"] if part == "jump" else []))
            x, y = col["%s.%s" % (name, part)], col[name + ".depth"]
            check_stats(d[part], x, bins)
            check_stats(d["depth"], y, bins)
            ok = ~np.isnan(x)
            assert np.array_equal(ok, ~np.isnan(y))
            xe, ye = np.histogram_bin_edges(x[ok], bins), np.histogram_bin_edges(y[ok], bins)
            c2 = np.histogram2d(x[ok], y[ok], (xe, ye))[0].astype(np.int64)
            same(d["hist2d"], (c2, xe, ye), (s, name, "hist2d"))
            xi, yi = np.unravel_index(np.argmax(c2), c2.shape)
            assert d["mode"] == (((xe[:-1] + xe[1:]) / 2.)[xi], ((ye[:-1] + ye[1:]) / 2.)[yi])
        for name, c in (("lvz", "lvz.depth"), ("step", "step.depth"), ("basement", "basement")):
            n = int(np.sum(~np.isnan(col[c])))
            assert r[s][name]["probability"] == n / int(sel.sum()) and 0.05 < r[s][name]["probability"] < 0.95
        assert "probability" not in r[s]["upper"] and "probability" not in r[s]["slow"]
    one = bh.posterior_features(rows[site == 1], {k: tuple(np.asarray(v)[1] if np.ndim(v) else v for v in f) for k, f in FEATURES.items()},
                                bins=bins, quantiles=QS, engine=engine)                      # no site: one dict, the same bits
    same(one, r[1])
    assert "quantiles" not in bh.posterior_features(rows, dict(m=("vsmean", 0, 10)), engine=engine)["m"]
    with pytest.raises(ValueError, match="'m', site 0.*z0 < z1"):
        bh.posterior_features(rows, dict(m=("vsmean", 10, 10)), engine=engine)


def test_a_site_without_rows_or_without_the_feature_has_empty_statistics(engine):
    import bayhunter_amd as bh
    rows = np.array([row_of([3.0, 3.5], [10.0], np.float32, 4), row_of([3.5], [], np.float32, 4)])
    r = bh.posterior_features(rows, dict(lvz=("drop", 0, 50), m=("vsmean", 0, 20), n=("nifaces", 0, 50)), site=np.array([0, 0], np.int32),
                              nsites=2, quantiles=(0.5,), engine=engine)
    assert r[0]["rows"] == 2 and r[1]["rows"] == 0
    assert r[0]["lvz"]["probability"] == 0.0 and np.isnan(r[1]["lvz"]["probability"])
    for d in (r[0]["lvz"]["depth"], r[0]["lvz"]["jump"], r[1]["m"], r[1]["n"]):
        assert d["count"] == 0 and np.isnan([d["median"], d["mean"], d["min"], d["mode"], d["quantiles"][0]]).all()
        assert not d["hist"][0].any() and not d["constant"]
    assert not r[0]["lvz"]["hist2d"][0].any() and np.isnan(r[0]["lvz"]["mode"]).all()
    assert (r[0]["m"]["count"], r[0]["m"]["min"], r[0]["m"]["max"]) == (2, 3.25, 3.5)
    assert (r[0]["n"]["min"], r[0]["n"]["max"]) == (0.0, 1.0) and np.array_equal(r[0]["n"]["hist"][0], [1, 1])


def test_the_covariance_takes_the_features_as_it_takes_the_same_columns(three_sites, engine):
    import bayhunter_amd as bh
    rows, site, ref = three_sites
    dep = np.linspace(0, 60, 7)
    pick = dict(upper=FEATURES["upper"], step=FEATURES["step"], basement=FEATURES["basement"], crustal=FEATURES["crustal"])
    cols = {name: ref[LABELS.index(name)] for name in ("upper", "step.depth", "step.jump", "basement", "crustal")}
    a = bh.posterior_covariance(rows, site, dep_int=dep, features=pick, engine=engine)
    b = bh.posterior_covariance(rows, site, dep_int=dep, columns=cols, engine=engine)
    for s in range(3):
        assert a[s]["names"] == [float(d) for d in dep] + ["upper", "step.depth", "step.jump", "basement", "crustal"] == b[s]["names"]
        gone = np.isnan(np.array(list(cols.values()))[:, site == s]).any(0).sum()
        assert a[s]["masked"] == gone and 0 < a[s]["n"] == (site == s).sum() - gone and gone > 50      # listwise deletion
        same(a[s], b[s], (s,))
    with pytest.raises(ValueError, match="one set"):
        bh.posterior_covariance(rows, site, features=pick, moho=(5.0, 30.0), engine=engine)
    with pytest.raises(ValueError, match="one set"):
        bh.posterior_covariance(rows, site, features=pick, columns=dict(x=np.zeros(len(rows))), engine=engine)


# ---- refusals --------------------------------------------------------------------------------------------------------------

def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def test_refusals_through_the_c_abi_leave_the_handle_usable(engine):
    from bayhunter_amd import engine as E
    L = engine._L
    rows, site, par, ref = case(4, np.float64, 257, "a")
    ld = loaded(rows, site, engine, S4)
    bare = loaded(rows, site, engine, S4, scalars=False)

    def refused(rc, text):
        assert rc == E.BH_EINVAL
        with pytest.raises(E.EngineError, match=text):
            engine._check(rc)

    def call(h, kinds, p, found=None):
        kinds, p = np.ascontiguousarray(kinds, np.int32), np.ascontiguousarray(p, np.float64)
        return L.bh_posterior_features(h._p, kinds.size, _ptr(kinds), _ptr(p), _ptr(found) if found is not None else None)

    try:
        one = par[:, :1].copy()
        off, ok, cnt = np.arange(0, 2 * S4 + 1, 2, dtype=np.int64), np.tile([0.0, 1.0], S4), np.zeros(S4, np.uint32)
        rk = np.zeros((S4, 1, 1), np.uint32)
        # the set before it exists
        refused(L.bh_posterior_scalar_cols(ld._p, E.SCALARS_FEATURES, _ptr(np.zeros(1, np.int32))), "FEATURES set does not exist yet")
        refused(L.bh_posterior_scalar_hist(ld._p, E.SCALARS_FEATURES, 0, _ptr(off), _ptr(ok), _ptr(cnt)), "does not exist yet")
        qlo, qup = rk.astype(np.uint64), rk.astype(np.uint64)
        refused(L.bh_posterior_scalar_quantiles(ld._p, E.SCALARS_FEATURES, 1, _ptr(rk), _ptr(qlo), _ptr(qup)), "does not exist yet")
        refused(L.bh_posterior_scalar_hist(ld._p, 2, 0, _ptr(off), _ptr(ok), _ptr(cnt)), "no such scalar set")
        dep, c0 = np.array([10.0]), np.zeros(1, np.int32)
        cov = lambda which: L.bh_posterior_cov(ld._p, 1, _ptr(dep), which, 1, _ptr(c0), *([None] * 10))   # noqa: E731
        refused(cov(E.SCALARS_FEATURES), "FEATURES set does not exist yet")
        refused(cov(-1), "BH_SCALARS_MOHO or BH_SCALARS_USER")
        refused(cov(3), "BH_SCALARS_MOHO or BH_SCALARS_USER")
        found = np.full((S4, 1), -7, np.int64)
        refused(call(ld, [9], one, found), r"kind\[0\]")
        refused(call(ld, [0, -1], par[:, :2], found), r"kind\[1\]")
        refused(L.bh_posterior_features(ld._p, 0, _ptr(np.zeros(1, np.int32)), _ptr(one), None), "F: 1..64")
        refused(L.bh_posterior_features(ld._p, 65, _ptr(np.zeros(65, np.int32)), _ptr(np.tile(one, (1, 65, 1))), None), "F: 1..64")
        k65 = np.array([E.FEATURE_DROP] * 32 + [E.FEATURE_TTS], np.int32)                   # 65 columns
        refused(call(ld, k65, np.tile(one, (1, 33, 1)), None), "BH_SCALARS_MAXCOLS")
        for s, i, v, text in ((2, 1, 5.0, r"par\[2\]\[0\].*z0 < z1"), (1, 1, 4.0, r"par\[1\]\[0\].*z0 < z1"), (3, 0, np.nan, r"par\[3\]\[0\].*finite"),
                              (0, 2, np.inf, r"par\[0\]\[0\].*finite"), (0, 0, -0.25, r"par\[0\]\[0\].*below 0")):
            p = one.copy()
            p[:, 0, :2] = (5.0, 30.0)
            p[s, 0, i] = v
            refused(call(ld, [0], p, found), text)
        p = par[:, 5:7].copy()
        p[1, 1, 2] = -0.5
        refused(call(ld, [E.FEATURE_DROP, E.FEATURE_JUMP], p, found), r"par\[1\]\[1\].*negative")
        refused(call(bare, [0], one, found), "bh_posterior_keep_rows")
        assert (found == -7).all()
        refused(L.bh_posterior_scalar_cols(ld._p, E.SCALARS_FEATURES, _ptr(np.zeros(1, np.int32))), "does not exist yet")
        # the same handle still works; a set formed again replaces the one before
        ld.features(np.arange(9), par)
        assert np.array_equal(gathered(ld, E.SCALARS_FEATURES, len(rows), 13)[0], ref, equal_nan=True)
        f = ld.features([E.FEATURE_NIFACES], par[:, 8:9])
        q = np.zeros(1, np.int32)
        engine._check(L.bh_posterior_scalar_cols(ld._p, E.SCALARS_FEATURES, _ptr(q)))
        assert q[0] == 1 and np.array_equal(f[:, 0], ld.rows)
        assert np.array_equal(gathered(ld, E.SCALARS_FEATURES, len(rows), 1)[0][0], ref[12])
        assert ld.cov(dep, E.SCALARS_FEATURES, [0])["n"].sum() == len(rows)
        refused(L.bh_posterior_scalar_hist(ld._p, E.SCALARS_FEATURES, 1, _ptr(off), _ptr(ok), _ptr(cnt)), "column out of range")
    finally:
        ld.close()
        bare.close()


# ---- the callers -----------------------------------------------------------------------------------------------------------

def test_chains_form_the_features_of_their_device_record(tmp_path, engine):
    """2 sites x 4 chains under their own priors, 100 kept iterations each (the run of tests/test_gpu_posterior_cov.py): the
    features from the device store equal those of the function on the host arrays of samples(site=s)"""
    import bayhunter_amd as bh
    from bayhunter_amd.device_chains import DeviceChains
    from test_gpu_posterior_scalars import site_targets
    from test_gpu_sites_priors import SITE_INIT, SITE_PRIORS
    T, Cn = 100, 4
    inits = [dict(SITE_INIT[s], iter_burnin=100, iter_main=T, maxmodels=T, savepath=str(tmp_path)) for s in range(2)]
    dc = DeviceChains(site_targets(), Cn, inits, SITE_PRIORS[:2], seed=78, search="fast", record="device").run()
    assert dc.thinning == 1 and dc.nsamples("p2") == T
    n = T * Cn
    feats = dict(crust=("vsmean", 0, [20.0, 25.0]), lvz=("drop", 0, 60, 0.05), moho=("above", [5.0, 8.0], 55, [3.6, 3.8]),
                 n40=("nifaces", 0, 40), slow=("vsmin", 0, 30))
    a = dc.posterior_features(feats, bins=20, quantiles=(0.16, 0.84))
    ex = dc.posterior_features(feats, exclude_chains=(1, 6))
    cv = dc.posterior_covariance(dep_int=[10.0, 30.0], features=dict(crust=feats["crust"], n40=feats["n40"]))
    for s in range(2):
        own = {k: tuple(np.asarray(v)[s] if np.ndim(v) else v for v in f) for k, f in feats.items()}
        h = dc.samples("p2", site=s)
        m = h["models"].reshape(n, -1)
        assert a[s]["rows"] == n and a[s]["dropped"] == 0 and a[s]["crust"]["count"] == n
        same(a[s], bh.posterior_features(m, own, bins=20, quantiles=(0.16, 0.84), engine=engine), (s, "features"))
        keep = np.ones(Cn, bool)
        keep[[1] if s == 0 else [2]] = False                               # chains 1 | 6
        mk = h["models"][:, keep].reshape(T * 3, -1)
        want = bh.posterior_features(mk, own, engine=engine)
        assert ex[s]["dropped"] == 2 * T and ex[s]["rows"] == len(mk)
        ex[s].pop("dropped"), want.pop("dropped")
        same(ex[s], want, (s, "excluded"))
        same(cv[s], bh.posterior_covariance(m, dep_int=[10.0, 30.0], features=dict(crust=own["crust"], n40=own["n40"]), engine=engine),
             (s, "covariance"))
        assert cv[s]["names"] == [10.0, 30.0, "crust", "n40"]
    host = DeviceChains(site_targets(), Cn, inits, SITE_PRIORS[:2], seed=78, search="fast", record="host")
    with pytest.raises(Exception, match="record='device'"):
        host.posterior_features(feats)


def test_features_from_storage_reads_every_stations_files(tmp_path, engine):
    import bayhunter_amd as bh
    rs = np.random.RandomState(12)
    sets = [make_rows(rs, 300, 12, np.float32, "b").astype(np.float64), make_rows(rs, 200, 6, np.float32, "b").astype(np.float64)]
    paths = []
    for s, m in enumerate(sets):
        d = tmp_path / ("st%d" % s) / "data"
        d.mkdir(parents=True)
        np.save(str(d / "c_models.npy"), m)
        paths.append(str(d))
    feats = dict(top=("vstime", 0, [1.0, 2.0]), lvz=("drop", 5, 60, [0.8, 0.6]), n=("nifaces", 0, 30))
    r = bh.features_from_storage(paths, feats, bins=25, quantiles=(0.5,), engine=engine)
    for s in range(2):
        own = {k: tuple(np.asarray(v)[s] if np.ndim(v) else v for v in f) for k, f in feats.items()}
        assert r[s]["rows"] == len(sets[s]) and 0.1 < r[s]["lvz"]["probability"] < 0.9
        same(r[s], bh.posterior_features(sets[s], own, bins=25, quantiles=(0.5,), engine=engine), (s,))
