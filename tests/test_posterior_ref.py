"""tests/posterior_ref.py (the GPU tests' oracle) against the reference's own posterior outputs
(tests/golden/posterior_golden.npz): bit for bit for the interpolated vs, median, min, max, mode and histograms; the
mean and std of the reference and of the engine's rule against exact rationals.  CPU only."""
import math

import numpy as np
import pytest

from conftest import golden
import posterior_ref as R

KEYS = ("f32", "f64of32", "f64")


@pytest.fixture(scope="module")
def G():
    return golden("posterior_golden.npz")


@pytest.mark.parametrize("key", KEYS)
def test_interpolated_vs_is_the_references_bit_for_bit(G, key):
    vsi = R.interp(G[key + "_models"], G["dep_int"])
    assert vsi.shape == G[key + "_vsi"].shape
    assert np.array_equal(vsi, G[key + "_vsi"])


@pytest.mark.parametrize("key", KEYS)
def test_fixture_holds_the_edge_cases(G, key):
    m = G[key + "_models"]
    vs, d, di, n = R.depths(m)
    assert (n == 1).sum() > 100                                   # one-layer rows
    assert np.isnan(m).all(1).sum() > 10                          # NaN-only rows (dropped)
    if key != "f64":
        assert (np.nan_to_num(d[:, 0], nan=-1) == 0).sum() > 10    # first interface at depth 0
        assert (np.diff(d, axis=1) == 0).sum() > 10               # zero-thickness layers
        on_grid = np.isin(d, G["dep_int"]).sum()
        assert on_grid > 500                                      # interfaces exactly on grid depths
    # d is not zd: the cumulative sum rounds differently (general float64 rows; float32 values sum exactly in float64)
    if key == "f64":
        ok = ~np.isnan(m).all(1)
        mm = m[ok]
        zd = np.full(d.shape, np.nan)
        for i in range(len(mm)):
            k = n[i]
            z = mm[i, k:2 * k]
            zd[i, :k - 1] = (z[:-1] + z[1:]) / 2.
        assert np.sum(np.any((d != zd) & ~np.isnan(d), axis=1)) > 10


@pytest.mark.parametrize("key", KEYS)
def test_exact_statistics_are_the_references(G, key):
    s = R.singlemodels(G[key + "_models"], G["dep_int"])
    assert np.array_equal(s["median"], G[key + "_median"])
    assert np.array_equal(s["min"], G[key + "_min"])
    assert np.array_equal(s["max"], G[key + "_max"])
    assert s["mode_valid"]
    assert np.array_equal(s["mode"], G[key + "_mode"])
    assert np.array_equal(s["dep_center"], G[key + "_dep_center"])
    vsi = s["vsi"]
    e = np.linspace(vsi.min(), vsi.max(), int((vsi.max() - vsi.min()) / 0.025) + 1)
    assert np.array_equal(R.hist2d(vsi, G["dep_int"], e, G["dep_int"]), G[key + "_modecounts"])


@pytest.mark.parametrize("key", KEYS)
def test_reference_mean_and_std_are_within_1e13_of_exact(G, key):
    vsi = G[key + "_vsi"]
    for j in range(0, vsi.shape[1], 10):
        m, var = R.exact_mean_std(vsi[:, j])
        assert abs(G[key + "_mean"][j] - float(m)) <= 1e-13 * abs(float(m))
        std = math.sqrt(float(var))
        assert abs(G[key + "_std"][j] - std) <= 1e-13 * std + (0 if std else 0)


@pytest.mark.parametrize("key", KEYS)
def test_2d_plot_histograms_are_the_references(G, key):
    from bayhunter_amd.posterior import hist2d_edges
    m = G[key + "_models"]
    samples, depbins, _ = hist2d_edges(None, None, np.arange(0, 61, 1.))
    assert np.array_equal(samples, G[key + "_h2_samples"]) and np.array_equal(depbins, G[key + "_h2_depbins"])
    vsi = R.interp(m, samples)
    _, _, vse = hist2d_edges(vsi.min(), vsi.max(), np.arange(0, 61, 1.))
    assert np.array_equal(vse, G[key + "_h2_vsedges"])
    assert np.array_equal(R.hist2d(vsi, samples, vse, depbins), G[key + "_h2_counts"])
    assert np.array_equal(R.interface_hist(m, depbins), G[key + "_h2_interfaces"])


@pytest.mark.parametrize("key", KEYS)
def test_best_misfit_step_model_is_the_references(G, key):
    from bayhunter_amd.posterior import stepmodel
    m, mis = G[key + "_models"], G[key + "_misfits"]
    vs, dep = stepmodel(m[np.argmin(mis)])
    assert np.array_equal(vs, G[key + "_best_vs"]) and vs.dtype == G[key + "_best_vs"].dtype
    assert np.array_equal(dep, G[key + "_best_dep"])


def test_restatement_rejects_a_row_that_is_not_a_prefix():
    m = np.array([[3.0, 4.0, 1.0, 5.0], [3.0, np.nan, 1.0, np.nan]])
    with pytest.raises(ValueError):
        R.split(m)


# ---- the exact integer sums, the scale rule and the extended-precision std (the oracle of tests/test_gpu_posterior_paths.py) ----

def _ulp_apart(got, want):
    """|got - want| in ulps of the larger of the two, `want` a Fraction."""
    from fractions import Fraction
    return abs(Fraction(got) - want) / Fraction(math.ulp(max(got, float(want))))


@pytest.mark.parametrize("key", KEYS)
def test_integer_sums_give_the_exact_mean_and_std_of_the_golden_columns(G, key):
    from bayhunter_amd.posterior import _mean_std
    vsi = G[key + "_vsi"]
    n, D = vsi.shape
    scale, x0, exact = R.scale_rule(vsi)
    assert all(exact)
    low = R.low_bit(vsi)
    assert scale == [int(v) for v in low.min(0)]
    s1, s2 = R.int_sums(vsi, scale, x0)
    if key != "f64":
        assert max(s1) < n << 25              # float32 values: every Y is below 2^25
    for j in range(D):
        mean, std = R.exact_mean(n, s1[j], scale[j], x0[j]), R.exact_std(n, s1[j], s2[j], scale[j])
        assert abs(G[key + "_mean"][j] - float(mean)) <= 1e-13 * abs(float(mean))
        assert abs(G[key + "_std"][j] - float(std)) <= 1e-13 * float(std)
        m, s = _mean_std(n, [s1[j] & 0xffffffff, s1[j] >> 32] + [(s2[j] >> (32 * i)) & 0xffffffff for i in range(4)], scale[j], x0[j])
        assert m == float(mean)                # int / int is correctly rounded
        assert (s == 0.0) if std == 0 else _ulp_apart(s, std) <= 1
    for j in range(0, D, 10):                  # ... and the sums are those of the values themselves
        m, var = R.exact_mean_std(vsi[:, j])
        assert m == R.exact_mean(n, s1[j], scale[j], x0[j])
        std = R.exact_std(n, s1[j], s2[j], scale[j])
        assert std * std <= var and var * (1 - 2.0 ** -98) <= std * std * (1 + 2.0 ** -98)


def test_scale_rule_and_sums_of_hand_made_columns():
    from fractions import Fraction
    z = np.zeros((5, 1))
    assert R.low_bit(z).min() == R.NO_BIT
    assert R.scale_rule(z) == ([0], [0], [1])
    assert R.int_sums(z, [0], [0]) == ([0], [0])
    assert R.exact_std(5, 0, 0, 0) == 0
    assert [int(v) for v in R.low_bit(np.array([1.0, 3.0, 0.75, -6.0, 2.0 ** -1074, 2.0 ** -1060 * 3]))] == [0, 0, -2, 1, -1074, -1060]
    # 4.0 beside 2^-70: the scale is raised until 4.0 * 2^-scale < 2^62, and 2^-70 rounds to 0
    c = np.array([[4.0], [2.0 ** -70], [4.0]])
    assert R.scale_rule(c) == ([-59], [0], [0])
    s1, s2 = R.int_sums(c, [-59], [0])
    assert (s1, s2) == ([2 << 61], [2 << 122])
    assert R.exact_mean(3, s1[0], -59, 0) == Fraction(8, 3)
    assert float(R.exact_std(3, s1[0], s2[0], -59)) == math.sqrt(32 / 9.)
    # two values one ulp apart: Y is 0 or 1, the mean lies between them and the std is half an ulp (or sqrt(2) / 3 of it)
    a = 3.3
    b = np.nextafter(a, 4.0)
    u = Fraction(b) - Fraction(a)
    c = np.array([[a, a], [b, b], [a, b]])
    scale, x0, exact = R.scale_rule(c)
    assert scale == [-51, -51] and exact == [1, 1] and x0 == [int(Fraction(a) / u)] * 2
    s1, s2 = R.int_sums(c, scale, x0)
    assert (s1, s2) == ([1, 2], [1, 2])
    assert R.exact_mean(3, 2, -51, x0[0]) == Fraction(a) + 2 * u / 3
    assert R.exact_std(2, 1, 1, -51) == u / 2
    std = R.exact_std(3, 1, 1, -51)
    assert std * std <= 2 * u * u / 9 <= std * std * (1 + Fraction(1, 1 << 98))
    # large offsets: Y up to 2^62 - 1 uses every limb
    c = np.array([[-2.0 ** 61], [2.0 ** 61 - 512.0], [1.0]])
    scale, x0, exact = R.scale_rule(c)
    assert (scale, x0, exact) == ([0], [-1 << 61], [1])
    s1, s2 = R.int_sums(c, scale, x0)
    ys = [0, (1 << 62) - 512, (1 << 61) + 1]
    assert (s1, s2) == ([sum(ys)], [sum(y * y for y in ys)])
