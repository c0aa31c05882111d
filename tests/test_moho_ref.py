"""The restatement tests/moho_ref.py against the reference's own outputs (tests/golden/moho_golden.npz, written by
tests/golden/gen_moho_golden.py from PlotFromStorage.plot_moho_crustvel_tradeoff and plot_posterior_*): the per-row arrays,
counts, medians and histogram counts bit for bit; and the host-side edge builders of bayhunter_amd/posterior.py against
numpy's.  No GPU."""
import numpy as np
import pytest

from conftest import golden
import moho_ref as MR

KEYS = ("f32", "f64of32", "f64")


@pytest.fixture(scope="module")
def G():
    return golden("moho_golden.npz")


def test_np_sum_is_numpys_order():
    rs = np.random.RandomState(1)
    for _ in range(4000):
        a = rs.uniform(-1, 1, rs.randint(1, 33)) * 10.0 ** rs.randint(-8, 8)
        assert MR.np_sum(a) == np.sum(a)


@pytest.mark.parametrize("key", KEYS)
def test_rows_are_the_references(G, key):
    rows = MR.moho_rows(G[key + "_models"], float(G["lo"]), float(G["hi"]), float(G["mohovs"]))
    found = ~np.isnan(rows[:, 3])
    assert np.array_equal(np.isnan(rows[:, 0]), ~found)
    assert np.array_equal(rows[found], G[key + "_values"])            # every row: moho, vslast, vscrust, vsjump
    assert found.sum() / float(len(rows)) == float(G[key + "_share"]) >= 1. / 3.


@pytest.mark.parametrize("key", KEYS)
def test_sets_hold_the_cases_of_the_rule(G, key):
    m = G[key + "_models"]
    lo, hi, mv = float(G["lo"]), float(G["hi"]), float(G["mohovs"])
    rows = MR.moho_rows(m, lo, hi, mv)
    import posterior_ref as R
    vs, d, _, n = R.depths(m)
    found = ~np.isnan(rows[:, 0])
    k = np.array([np.flatnonzero(d[i] == rows[i, 0])[0] + 1 if found[i] else 0 for i in range(len(rows))])   # crustal layers
    for want in (lambda c: (c > 0) & (c < 8), lambda c: c == 8, lambda c: (c > 8) & (c < 16), lambda c: c == 16, lambda c: c > 16):
        assert want(k).sum() >= 10
    assert (n == 1).sum() >= 10 and np.isnan(m).all(1).sum() >= 10
    assert (np.nan_to_num(vs[:, 0]) > mv).sum() >= 10
    assert (np.diff(np.nan_to_num(d, nan=-1.0), axis=1) == 0).any(1).sum() >= 10     # zero-thickness layers
    at = np.float64(mv if key == "f64" else np.float32(mv))     # a vs exactly mohovs (the float32 sets: the float32 next to it)
    assert (vs.astype(np.float64) == at).any(1).sum() >= 10
    assert (d == lo).any(1).sum() >= 10 and (d == hi).any(1).sum() >= 10
    inside = (d > lo) & (d < hi)
    assert ((inside.sum(1) > 0) & ~found).sum() >= 10                             # candidates that fail the vs test


@pytest.mark.parametrize("key", KEYS)
def test_medians_and_histograms_are_the_references(G, key):
    s = MR.moho_summary(G[key + "_models"], float(G["lo"]), float(G["hi"]), float(G["mohovs"]), int(G["bins"]))
    assert s["count"] == len(G[key + "_values"])
    for q, name in enumerate(MR.COLUMNS):
        assert s[name]["median"] == G[key + "_medians"][q]
        assert np.array_equal(s["hist"][name][0], G[key + "_hist"][q])
        assert s["hist"][name][0].sum() == s["count"]
    for i, name in enumerate(MR.COLUMNS[1:]):
        assert np.array_equal(s["hist2d"][name][0], G[key + "_hist2d"][i])
        xe, ye = s["hist2d"][name][1:]
        c, xe2, ye2 = np.histogram2d(s["values"][:, i + 1], s["values"][:, 0], bins=int(G["bins"]))
        assert np.array_equal(xe, xe2) and np.array_equal(ye, ye2) and np.array_equal(c, s["hist2d"][name][0])
        xi, yi = np.unravel_index(c.argmax(), c.shape)
        assert s["mode"][name] == (((xe[:-1] + xe[1:]) / 2.)[xi], ((ye[:-1] + ye[1:]) / 2.)[yi])


def scalar_columns(G):
    """(golden key, column) of every axis of the reference's scalar plots"""
    nl = MR.nlayers(G["sc_models"])
    cols = [("likes_0", G["sc_likes"], False), ("misfits_0", G["sc_misfits"][:, 0], False),
            ("misfits_1", G["sc_misfits"][:, 1], False), ("vpvs_0", G["sc_vpvs"], False)]
    cols += [("noise_%d" % i, G["sc_noise"][:, i], False) for i in range(4)]
    cols += [("others_0", G["sc_likes"], False), ("others_1", G["sc_misfits"][:, -1], False), ("others_2", G["sc_vpvs"], False)]
    return cols, nl


def test_scalar_posteriors_are_the_references(G):
    cols, nl = scalar_columns(G)
    for key, v, _ in cols:
        s = MR.scalar_summary(v)
        assert np.array_equal(s["hist"][0], G["sc_%s_hist" % key]), key
        assert s["median"] == float(G["sc_%s_median" % key]), key
        assert s["constant"] == (key in ("noise_0", "noise_2"))
    for key in ("nlayers_0", "others_3"):
        s = MR.scalar_summary(nl, nlayer_edges=True)
        assert np.array_equal(s["hist"][0], G["sc_%s_hist" % key]) and s["median"] == float(G["sc_%s_median" % key])
        assert s["hist"][0].sum() == len(G["sc_models"])


def test_host_edge_builders_are_numpys():
    from bayhunter_amd.posterior import moho_edges, scalar_edges, median_of_middles
    rs = np.random.RandomState(2)
    for dt in (np.float32, np.float64):
        for _ in range(50):
            v = (rs.normal(0, 1, rs.randint(1, 40)) * 10.0 ** rs.randint(-3, 4)).astype(dt)
            if rs.randint(3) == 0:
                v[:] = v[0]
            e = scalar_edges(v.min(), v.max(), dt, 20)
            if v.min() == v.max():
                m = float(v[0])
                assert np.array_equal(e, np.array([m - 1, m - 0.1, m + 0.1, m + 1]))
            else:
                ref = np.histogram_bin_edges(v, 20)
                assert e.dtype == ref.dtype and np.array_equal(e, ref)
            s = np.sort(v)
            n = len(s)
            got = median_of_middles(s[(n - 1) // 2], s[min((n - 1) // 2 + 1, n - 1)], n, dt)
            assert got == np.median(v) and type(got) is dt
            v64 = v.astype(np.float64)
            assert np.array_equal(moho_edges(v64.min(), v64.max(), 50), np.histogram_bin_edges(v64, 50))
            assert np.array_equal(moho_edges(v64.min(), v64.max(), 50), np.histogram2d(v64, v64, bins=50)[1])
    nl = np.array([0., 3., 5., 5., 2.])
    assert np.array_equal(scalar_edges(nl.min(), nl.max(), np.float64, 20, nlayers=True), np.arange(0, 7) - 0.5)
    assert np.array_equal(moho_edges(np.nan, np.nan, 50), np.histogram_bin_edges(np.zeros(0), 50))
    assert np.array_equal(scalar_edges(np.nan, np.nan, np.float32, 20), np.histogram_bin_edges(np.zeros(0, np.float32), 20))


def test_public_functions_refuse_without_a_range():
    from bayhunter_amd import posterior_moho
    with pytest.raises(ValueError, match="priors"):
        posterior_moho(np.zeros((1, 4)), moho=None)


def test_scalar_columns_may_not_take_the_results_own_keys():
    from bayhunter_amd import posterior_scalars
    m = np.zeros((2, 4))
    for name in ("rows", "invalid_rows", "dropped", "nlayers"):
        with pytest.raises(ValueError, match=name):
            posterior_scalars(m, {name: np.zeros(2)})


def test_exact_moments_leave_nan_out():
    from fractions import Fraction
    m, var = MR.exact_mean_std(np.array([0.1, np.nan, 0.3], np.float64))
    assert m == (Fraction(0.1) + Fraction(0.3)) / 2 and var == ((Fraction(0.1) - m) ** 2 + (Fraction(0.3) - m) ** 2) / 2
