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
