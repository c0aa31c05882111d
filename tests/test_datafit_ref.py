"""The numpy restatement of the posterior data fits (tests/datafit_ref.py) against the reference's own outputs in
tests/golden/datafit_golden.npz, the quantile formula against numpy.quantile, and the pure host parts of
bayhunter_amd/datafits.py (quantile ranks and interpolation, the planner of site groups and forward batches).  No GPU."""
import numpy as np
import pytest

from conftest import golden
import datafit_ref as DR

KEYS = ("f32", "f64of32", "f64")
DEFAULT_Q = (0.025, 0.16, 0.5, 0.84, 0.975)


@pytest.fixture(scope="module")
def G():
    return golden("datafit_golden.npz")


def bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("tag", ("plain", "mantle"))
def test_layer_rule_is_the_references(G, key, tag):
    rows, vpvs = G[key + "_rows"], G[key + "_vpvs"]
    mantle = None if tag == "plain" else tuple(G["mantle"])
    want = {k: G["%s_%s_%s" % (key, tag, k)] for k in ("vp", "vs", "rho", "h", "nlay")}
    assert rows.dtype == vpvs.dtype == (np.float32 if key == "f32" else np.float64)
    assert sorted(set(want["nlay"])) == list(range(1, 22))
    deep = 0
    for i, (row, k) in enumerate(zip(rows, vpvs)):
        vp, vs, h, rho = DR.layers(row, k, mantle)
        n = want["nlay"][i]
        assert len(vs) == n
        for name, got in (("vp", vp), ("vs", vs), ("rho", rho), ("h", h)):
            assert bits_equal(got, want[name][i, :n]), (key, tag, i, name)
        assert h[n - 1] == 0.0
        deep += int(mantle is not None and np.any(vp != vs * row.dtype.type(k)))
    assert (deep > 10) == (tag == "mantle")
    # the layer-major batch the engine takes is the same numbers widened, zeros beyond n
    nlay, h, vp, vs, rho = DR.layer_batch(rows, vpvs, mantle)
    assert np.array_equal(nlay, want["nlay"])
    for name, got in (("vp", vp), ("vs", vs), ("rho", rho), ("h", h)):
        assert bits_equal(got.T, want[name].astype(np.float64)), name


def test_vs_equal_to_mantle_vs_is_mantle_in_the_rows_dtype(G):
    """float32: vs = (float32)4.2 >= (float32)4.2; a float64 row holding that float32 value lies below the float64 4.2"""
    mv = float(G["mantle"][0])
    for key, hit in (("f32", True), ("f64of32", False)):
        rows, vpvs = G[key + "_rows"], G[key + "_vpvs"]
        i = [j for j, r in enumerate(rows) if r[2] == rows.dtype.type(np.float32(mv)) and not np.isnan(r[7]) and np.isnan(r[8])][0]
        vp = G[key + "_mantle_vp"][i]
        T = rows.dtype.type
        assert (vp[2] == T(rows[i, 2] * T(1.8))) == hit and (vp[2] == T(rows[i, 2] * T(vpvs[i]))) != hit


def test_best_of_chains_is_the_references_argmin(G):
    nch, outlier = int(G["best_nchains"]), int(G["best_outlier"])
    mis, chain, picks = G["best_misfits"], G["best_chain"], G["best_picks"]
    site = np.where(chain == outlier, -1, 0)                         # the outlier chain's rows take no part
    best = DR.best_of_chains(site, chain, mis, 1, nch)[0]
    start = np.concatenate(([0], np.cumsum(np.bincount(chain, minlength=nch))))
    for c in range(nch):
        assert best[c] == (-1 if c == outlier else start[c] + picks[c]), c
        if c != outlier:
            m = mis[chain == c]
            assert (m == m.min()).sum() > 1                         # (ties: the first one is picked)
    # the best of all: the first least among the chains' bests, as the reference's `<` keeps the earlier chain
    tb = DR.the_best(best, mis)
    assert mis[best[tb]] == mis[site == 0].min() and tb == min(c for c in range(nch) if c != outlier and mis[best[c]] == mis[best[tb]])
    # any row order gives the same rows
    perm = np.random.RandomState(3).permutation(len(mis))
    inv = np.argsort(perm)
    again = DR.best_of_chains(site[perm], chain[perm], mis[perm], 1, nch)[0]
    assert all((again[c] < 0 and best[c] < 0) or mis[perm][again[c]] == mis[best[c]] for c in range(nch))
    assert inv.size == mis.size


def columns(rs):
    out = []
    for n in (1, 2, 3, 100, 101):
        f32 = rs.normal(3.5, 0.4, n).astype(np.float32).astype(np.float64)
        gen = rs.normal(0.0, 1e-3, n)
        for v in (f32, gen):
            out.append(v)
            if n > 2:
                w = v.copy()
                w[rs.randint(0, n, n // 2)] = w[0]                  # repeats
                out.append(w)
    return out


def test_quantile_formula_is_numpys():
    from bayhunter_amd.datafits import quantile_rank, quantile_lerp
    rs = np.random.RandomState(101)
    for col in columns(rs):
        n = len(col)
        v = np.sort(col)
        for p in (0.0, 1.0, 0.5) + DEFAULT_Q:
            want = np.quantile(col, p, method="linear")
            got, a, b = DR.quantile(col, p)
            assert bits_equal(got, want), (n, p)
            k, g = quantile_rank(n, p)                              # the package's own ranks and interpolation
            assert (k, np.float64(g)) == DR.quantile_rank(n, p)
            assert v[k] == a and v[min(k + 1, n - 1)] == b
            assert bits_equal(quantile_lerp(a, b, g), want), (n, p)
        masked = np.concatenate((col, [np.nan, np.nan]))             # NaN is no value
        assert bits_equal(DR.quantile(masked, 0.16)[0], np.quantile(col, 0.16))
    assert np.isnan(DR.quantile(np.full(3, np.nan), 0.5)[0]) and quantile_rank(0, 0.5) == (0, 0.0)
    with pytest.raises(ValueError):
        quantile_rank(5, 1.5)


def test_masks_and_column_blocks():
    ncol = np.array([[5, 64], [3, 64], [5, 0]])
    assert list(DR.column_blocks(ncol)) == [0, 5, 69]
    y = np.arange(4 * 69, dtype=np.float64).reshape(4, 69)
    m = DR.masked(y, np.array([0, 0, 0, 1]), np.array([0, 1, 2, 0]), ncol)
    assert not np.isnan(m[0]).any() and np.array_equal(m[0], y[0])
    assert np.isnan(m[1, 3:5]).all() and not np.isnan(m[1, :3]).any() and not np.isnan(m[1, 5:]).any()
    assert np.isnan(m[2, 5:]).all() and not np.isnan(m[2, :5]).any()
    assert np.isnan(m[3]).all()
    s = DR.column_summary(m[:, 4], DEFAULT_Q)
    assert (s["count"], s["nan"], s["min"], s["max"]) == (2, 2, y[0, 4], y[2, 4])


def test_planner_loses_nothing_and_splits_no_site():
    from bayhunter_amd.datafits import plan_site_groups, plan_batches
    rs = np.random.RandomState(8)
    cases = [([0], 1, 1), ([5], 69, 10), ([3, 0, 0, 9], 4, 100), ([10] * 7, 8, 10 * 8 * 8 * 2), ([1000, 1, 1, 1000, 1], 10, 500)]
    cases += [(list(rs.randint(0, 2000, rs.randint(1, 40))), int(rs.randint(1, 300)), int(rs.randint(1, 1 << 22))) for _ in range(200)]
    split = 0
    for rows, ldy, budget in cases:
        groups = plan_site_groups(rows, ldy, budget)
        assert DR.plan_is_sound(rows, ldy, budget, groups), (rows, ldy, budget, groups)
        covered = [s for s0, s1 in groups for s in range(s0, s1)]
        assert covered == list(range(len(rows)))                     # nothing lost, nothing doubled, a site in one group
        split += len(groups) > 1
        # greedy: a group could not have taken the next site as well
        for (s0, s1) in groups[:-1]:
            assert sum(rows[s0:s1 + 1]) * ldy * 8 > budget
    assert split > 50
    assert plan_site_groups([], 3, 10) == []
    assert plan_site_groups([10, 10], 1, 1 << 40) == [(0, 2)]
    for n, b in ((0, 4), (1, 4), (4, 4), (5, 4), (8193, 1024)):
        bt = plan_batches(n, b)
        assert [r for r0, r1 in bt for r in range(r0, r1)] == list(range(n))
        assert all(0 < r1 - r0 <= b for r0, r1 in bt) and all(r1 - r0 == b for r0, r1 in bt[:-1])
    with pytest.raises(ValueError):
        plan_batches(3, 0)
    with pytest.raises(ValueError):
        plan_site_groups([1], 0, 10)


def test_saved_targets_come_back_from_a_config(tmp_path):
    """datafits_from_storage reads its targets from <station>_config.pkl"""
    import bayhunter_amd as bh
    from bayhunter_amd.results import save_config, saved_targets
    x = np.linspace(2, 40, 7)
    t1 = bh.RayleighDispersionPhase(x, 3.0 + 0.01 * x)
    t1.moddata.plugin.set_modelparams(mode=1, flsph=1)
    t2 = bh.PReceiverFunction(np.linspace(-5, 20, 64), np.zeros(64))
    t2.moddata.plugin.set_modelparams(gauss=1.5, p=7.1)
    d = tmp_path / "data"
    save_config([t1, t2], str(d / "st_config.pkl"), priors=dict(z=(0, 60), mantle=(4.3, 1.8)), initparams={})
    back = saved_targets(str(d))
    assert [type(t).__name__ for t in back] == ["RayleighDispersionPhase", "PReceiverFunction"]
    for t, t0 in zip(back, (t1, t2)):
        assert np.array_equal(t.obsdata.x, t0.obsdata.x) and np.array_equal(t.obsdata.y, t0.obsdata.y)
        assert t.moddata.plugin.modelparams == t0.moddata.plugin.modelparams and t.law() == "nocorr"


def test_stations_with_different_targets_become_slots():
    import bayhunter_amd as bh
    from bayhunter_amd.results import station_slots
    x = np.linspace(2, 40, 7)
    r, l = bh.RayleighDispersionPhase(x, 3 + 0 * x), bh.LoveDispersionPhase(x, 3 + 0 * x)
    p = bh.PReceiverFunction(np.arange(16) * 0.5 - 2, np.zeros(16))
    r2 = bh.RayleighDispersionPhase(x[:3], 3 + 0 * x[:3])
    rows, missing = station_slots([[r, p], [r2, p]])
    assert not missing and rows == [[r, p], [r2, p]]
    rows, missing = station_slots([[r, p], [l, r2], [p]])
    assert missing and rows == [[r, p, None], [r2, None, l], [None, p, None]]
    with pytest.raises(ValueError):
        station_slots([[r, r2]])
