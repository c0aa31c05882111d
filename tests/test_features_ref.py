"""tests/features_ref.py, the restatement of include/bh_engine_posterior_features.h that the GPU tests use as their oracle,
against things that are not the restatement: an integration of the package's own step model, tests/moho_ref.py (held to the
reference's outputs by tests/test_moho_ref.py), numpy's argmin / argmax of the differences, and rows built by hand for the ties."""
import math

import numpy as np
import pytest

import features_ref as FR
import moho_ref as MR


def row_of(vs, depths, dtype=np.float64, ML=None):
    """the row [vs.., z.., NaN..] whose interfaces (z_j + z_{j+1}) / 2 are `depths` (exact for dyadic depths)"""
    n = len(vs)
    ML = ML or n
    z = np.zeros(n)
    z[0] = depths[0] / 2 if n > 1 else 1.0
    for j in range(n - 1):
        z[j + 1] = 2 * depths[j] - z[j]
    row = np.full(2 * ML, np.nan)
    row[:n], row[n:2 * n] = vs, z
    return row.astype(dtype)


def dyadic_rows(rs, N, ML, dtype, step=0.25, top=40.0):
    rows = []
    for _ in range(N):
        n = rs.randint(1, ML + 1)
        dep = np.sort(rs.randint(1, int(top / step), n - 1)) * step
        vs = np.round(rs.uniform(1.0, 4.8, n) * 64) / 64
        rows.append(row_of(vs, dep, dtype, ML))
    return np.array(rows)


def test_row_of_gives_the_depths_it_was_asked_for():
    rs = np.random.RandomState(1)
    for dtype in (np.float32, np.float64):
        dep = np.sort(rs.randint(1, 160, 7)) * 0.25
        vs, d = FR.row_model(row_of(np.arange(8) + 1.0, dep, dtype, 10))
        assert np.array_equal(d, dep) and np.array_equal(vs, np.arange(8) + 1.0) and vs.dtype == dtype


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_window_averages_are_the_integrals_of_the_step_model(dtype):
    """vsmean, tts, vstime against a midpoint sum of the step model on a grid of 2^-10 km that hits every interface and both
    window edges: the two differ by the order of summation only (the grid's sum is math.fsum)"""
    from bayhunter_amd.posterior import stepmodel
    rs = np.random.RandomState(2)
    g = 2.0 ** -10
    rows = dyadic_rows(rs, 12, 9, dtype, step=2.0 ** -6, top=12.0)
    for i, row in enumerate(rows):
        z0 = rs.randint(0, 300) * 2.0 ** -6
        z1 = z0 + rs.randint(1, 500) * 2.0 ** -6
        if i == 0:
            z0, z1 = 13.0, 14.5                   # wholly inside the half-space
        vs_step, dep_step = stepmodel(row)
        x = z0 + (np.arange(int(round((z1 - z0) / g))) + 0.5) * g
        v = np.interp(x, dep_step, vs_step.astype(np.float64))
        mean = math.fsum(v * g) / (z1 - z0)
        tts = math.fsum(g / v)
        vs, d = FR.row_model(row)
        got = [FR.feature(k, vs, d, z0, z1, 0.0)[0] for k in ("vsmean", "tts", "vstime")]
        for a, b in zip(got, (mean, tts, (z1 - z0) / tts)):
            assert abs(a - b) <= 1e-12 * abs(b), (i, a, b)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_above_with_the_mohos_parameters_is_the_moho_depth(dtype):
    rs = np.random.RandomState(3)
    from test_gpu_posterior_scalars import crust_rows
    rows = crust_rows(rs, 300, ML=9, dtype=dtype)
    lo, hi, mv = 8.0, 41.0, 4.1
    want = MR.moho_rows(rows, lo, hi, mv)[:, 0]
    got = FR.features_ref(rows, ["above"], [[(lo, hi, mv)]])[0]
    assert 30 < np.isnan(want).sum() < 270
    assert np.array_equal(got, want, equal_nan=True)


def test_every_interface_counts_in_a_window_that_holds_them_all():
    rs = np.random.RandomState(4)
    from test_gpu_posterior_quantiles import synth
    rows = synth(rs, 200, 11, "f32")
    n = (~np.isnan(rows)).sum(1) // 2
    assert n.min() == 1 and n.max() == 11
    assert np.array_equal(FR.features_ref(rows, ["nifaces"], [[(0.0, 1e6, 0.0)]])[0], (n - 1).astype(np.float64))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_drop_and_jump_are_argmin_and_argmax_of_the_differences(dtype):
    rs = np.random.RandomState(5)
    from test_gpu_posterior_quantiles import synth
    rows = synth(rs, 300, 8, "f32" if dtype is np.float32 else "f64")
    t = FR.features_ref(rows, ["drop", "jump"], [[(0.0, 1e6, 0.0), (0.0, 1e6, 0.0)]])
    seen = [0, 0]
    for r, row in enumerate(rows):
        vs, d = FR.row_model(row)
        if len(vs) < 2:
            assert np.isnan(t[:, r]).all()
            continue
        df = np.diff(vs)
        assert df.dtype == dtype and len(set(df.tolist())) == len(df)        # distinct jumps: no tie rule at work
        k = int(np.argmin(df))
        if df[k] < 0:
            assert (t[0, r], t[1, r]) == (d[k], np.float64(df[k]))
            seen[0] += 1
        else:
            assert np.isnan(t[:2, r]).all()
        k = int(np.argmax(df))
        if df[k] > 0:
            assert (t[2, r], t[3, r]) == (d[k], np.float64(df[k]))
            seen[1] += 1
        else:
            assert np.isnan(t[2:, r]).all()
    assert min(seen) > 100


def test_thresholds_and_window_edges_are_strict():
    row = row_of([3.0, 2.5, 3.5, 3.0], [10.0, 20.0, 30.0])
    vs, d = FR.row_model(row)
    f = lambda k, z0, z1, c=0.0: FR.feature(k, vs, d, z0, z1, c)   # noqa: E731
    assert f("drop", 0, 50, 0.25) == (10.0, -0.5) and np.isnan(f("drop", 0, 50, 0.5)).all()        # jump < -c, strictly
    assert f("jump", 0, 50, 0.75) == (20.0, 1.0) and np.isnan(f("jump", 0, 50, 1.0)).all()
    assert f("drop", 10, 50) == (30.0, -0.5)
    assert np.isnan(f("drop", 10, 30)).all() and f("jump", 10, 30) == (20.0, 1.0)                    # an interface on an edge is outside
    assert f("nifaces", 10, 30) == (1.0,) and f("nifaces", 0, 30.25) == (3.0,) and f("nifaces", 30, 40) == (0.0,)
    assert f("above", 0, 50, 3.0) == (20.0,) and f("above", 0, 50, 2.5) == (20.0,) and f("above", 0, 50, 2.25) == (10.0,)
    assert np.isnan(f("above", 0, 50, 3.5)).all() and np.isnan(f("above", 20, 50, 3.25)).all()
    # a window wholly inside one layer, and wholly inside the half-space
    assert f("vsmean", 12, 18) == (2.5,) and f("vsmin", 12, 18) == (2.5, 12.0) and f("vsmax", 12, 18) == (2.5, 12.0)
    assert f("vsmean", 30, 90) == (3.0,) and f("tts", 30, 90) == (20.0,) and f("vsmin", 35, 90) == (3.0, 35.0)
    assert f("tts", 5, 25) == (np.float64(5.0) / 3.0 + 10.0 / 2.5 + 5.0 / 3.5,) and f("vstime", 0, 10) == (10.0 / (10.0 / 3.0),)
    # a layer that only touches the window has no length in it
    assert f("vsmin", 20, 30) == (3.5, 20.0) and f("vsmax", 10, 20) == (2.5, 10.0)


def test_ties_go_to_the_first():
    row = row_of([3.0, 2.5, 3.0, 2.5, 3.0, 3.0], [5.0, 10.0, 15.0, 20.0, 25.0])
    vs, d = FR.row_model(row)
    f = lambda k, z0, z1, c=0.0: FR.feature(k, vs, d, z0, z1, c)   # noqa: E731
    assert f("drop", 0, 50) == (5.0, -0.5) and f("drop", 5, 50) == (15.0, -0.5)
    assert f("jump", 0, 50) == (10.0, 0.5) and f("jump", 10, 50) == (20.0, 0.5)
    assert f("vsmin", 0, 50) == (2.5, 5.0) and f("vsmin", 7, 50) == (2.5, 7.0) and f("vsmin", 10, 50) == (2.5, 15.0)
    assert f("vsmax", 0, 50) == (3.0, 0.0) and f("vsmax", 5, 50) == (3.0, 10.0) and f("vsmax", 21, 50) == (3.0, 21.0)
    # zero-thickness layers are in no window, their interfaces are
    row = row_of([3.0, 1.0, 3.5, 9.0, 3.5], [10.0, 10.0, 20.0, 20.0])
    vs, d = FR.row_model(row)
    assert FR.feature("vsmin", vs, d, 0, 50, 0) == (3.0, 0.0) and FR.feature("vsmax", vs, d, 0, 50, 0) == (3.5, 10.0)
    assert FR.feature("nifaces", vs, d, 0, 50, 0) == (4.0,) and FR.feature("drop", vs, d, 0, 50, 0) == (20.0, -5.5)
    assert FR.feature("vsmean", vs, d, 0, 40, 0) == ((3.0 * 10 + 3.5 * 10 + 3.5 * 20) / 40,)


def test_a_half_space_alone_and_results_that_are_not_finite():
    vs, d = FR.row_model(row_of([3.5], [], ML=4))
    assert len(vs) == 1 and len(d) == 0
    for k in ("drop", "jump", "above"):
        assert np.isnan(FR.feature(k, vs, d, 0, 50, 0)).all()
    assert FR.feature("nifaces", vs, d, 0, 50, 0) == (0.0,) and FR.feature("vsmean", vs, d, 1, 3, 0) == (3.5,)
    assert FR.feature("vsmax", vs, d, 1, 3, 0) == (3.5, 1.0)
    vs, d = FR.row_model(row_of([0.0, 3.0], [10.0]))
    assert np.isnan(FR.feature("tts", vs, d, 0, 20, 0)).all() and FR.feature("vstime", vs, d, 0, 20, 0) == (0.0,)
    assert FR.feature("tts", vs, d, 10, 20, 0) == (10.0 / 3.0,)


def test_the_table_is_laid_out_feature_after_feature_with_every_sites_own_parameters():
    rows = np.array([row_of([2.0, 3.0, 4.5], [10.0, 30.0]), row_of([2.0, 3.0, 4.5], [10.0, 30.0])])
    par = [[(0, 20, 0), (0, 50, 0.5), (0, 50, 4.0)], [(0, 40, 0), (0, 50, 1.25), (0, 20, 4.0)]]
    t = FR.features_ref(rows, [FR.KINDS.index("vsmean"), "jump", "above"], par, site=[0, 1])
    assert t.shape == (4, 2)
    assert np.array_equal(t[:, 0], [2.5, 30.0, 1.5, 30.0])
    assert np.array_equal(t[:, 1], [(20 + 60 + 45) / 40, 30.0, 1.5, np.nan], equal_nan=True)
