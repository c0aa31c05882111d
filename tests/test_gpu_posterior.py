"""Posterior velocity-depth summaries on the GPU (bayhunter_amd/posterior.py, include/bh_engine_posterior.h) against the
restatement tests/posterior_ref.py, which tests/test_posterior_ref.py holds to the reference's own outputs: bit for bit
for min, max, median, mode and histograms; mean and std within 1e-13 of the exact rationals."""
import math

import numpy as np
import pytest

from conftest import golden
import posterior_ref as R

pytestmark = pytest.mark.gpu
KEYS = ("f32", "f64of32", "f64")


@pytest.fixture(scope="module")
def G():
    return golden("posterior_golden.npz")


def synth(rs, N, ML=21, dtype=np.float32):
    rows = np.full((N, 2 * ML), np.nan)
    n = rs.randint(1, ML + 1, N)
    for i in range(N):
        rows[i, :n[i]] = rs.uniform(2.0, 4.8, n[i])
        rows[i, n[i]:2 * n[i]] = np.sort(rs.uniform(0, 60, n[i]))
    return rows.astype(dtype)


def check_site(r, models, dep, exact_cols=10):
    vsi = R.interp(models, dep)
    assert r["count"] == len(vsi)
    assert np.array_equal(r["minmax"][0][0], vsi.min(0)) and np.array_equal(r["minmax"][0][1], vsi.max(0))
    assert np.array_equal(r["median"][0], R.median(vsi))
    vm, dc, ok = R.mode(vsi, dep)
    assert r["mode_valid"] == ok
    assert np.array_equal(r["mode"][0], vm, equal_nan=True) and np.array_equal(r["mode"][1], dc)
    mean, std = r["mean"][0], r["stdminmax"][0]
    for j in np.unique(np.linspace(0, dep.size - 1, exact_cols).astype(int)):
        m, var = R.exact_mean_std(vsi[:, j])
        assert abs(mean[j] - float(m)) <= 1e-13 * abs(float(m)), j
        s = math.sqrt(float(var))
        got = (std[1][j] - std[0][j]) / 2.
        if s == 0:
            assert std[0][j] == mean[j] == std[1][j]
        else:
            assert abs(got - s) <= 1e-13 * s + 4e-16 * abs(mean[j]), j


@pytest.mark.parametrize("key", KEYS)
def test_golden_sets_match_the_restatement(G, key, engine):
    from bayhunter_amd.posterior import posterior_models
    m = G[key + "_models"]
    r = posterior_models(m, dep_int=G["dep_int"], misfits=G[key + "_misfits"], engine=engine)
    check_site(r, m, G["dep_int"], exact_cols=21)
    assert np.array_equal(r["median"][0], G[key + "_median"])
    assert np.array_equal(r["mode"][0], G[key + "_mode"])
    assert np.all(np.abs(r["mean"][0] - G[key + "_mean"]) <= 1e-13 * G[key + "_mean"])
    vs, dep = r["minmisfit"]
    assert np.array_equal(vs, G[key + "_best_vs"]) and np.array_equal(dep, G[key + "_best_dep"])
    assert r["invalid_rows"] == 0


@pytest.mark.parametrize("key", KEYS)
def test_2d_plot_numbers_are_the_references(G, key, engine):
    from bayhunter_amd.posterior import posterior_hist2d
    h = posterior_hist2d(G[key + "_models"], dep_int=np.arange(0, 61, 1.), engine=engine)
    assert np.array_equal(h["vs_edges"], G[key + "_h2_vsedges"])
    assert np.array_equal(h["counts"], G[key + "_h2_counts"])
    assert np.array_equal(h["interfaces"], G[key + "_h2_interfaces"])


def test_edge_grids_and_constant_columns(engine):
    from bayhunter_amd.posterior import posterior_models
    rs = np.random.RandomState(5)
    m = synth(rs, 300, ML=6)
    m[:40] = np.nan
    m[:40, 0], m[:40, 1] = 3.5, 1.0                 # one-layer rows, vs 3.5
    for dep in (np.array([0.0, 7.5]), np.array([-5.0, 0.0, 0.25, 100.0, 300.0]), np.linspace(0, 100, 201)):
        check_site(posterior_models(m, dep_int=dep, engine=engine), m, dep)
    c = m[:40]                                      # a constant site: std 0 exactly, no mode bin
    r = posterior_models(c, dep_int=np.linspace(0, 10, 5), engine=engine)
    assert np.all(r["stdminmax"][0][0] == 3.5) and np.all(r["mean"][0] == 3.5)
    assert not r["mode_valid"] and np.all(np.isnan(r["mode"][0]))


def test_interleaved_sites_equal_each_site_alone_and_repeat_bit_for_bit(engine):
    from bayhunter_amd.posterior import posterior_models
    rs = np.random.RandomState(11)
    S = 64
    per = [synth(rs, 150 + 7 * s, dtype=(np.float32 if s % 2 else np.float64)).astype(np.float64) for s in range(S)]
    per[3] = per[3] + rs.uniform(-1e-7, 1e-7, per[3].shape)      # one site of general float64 values
    rows = np.concatenate(per)
    site = np.concatenate([np.full(len(p), s, np.int32) for s, p in enumerate(per)])
    perm = rs.permutation(len(rows))
    dep = np.linspace(0, 100, 201)
    a = posterior_models(rows[perm], site=site[perm], dep_int=dep, engine=engine)
    b = posterior_models(rows[perm], site=site[perm], dep_int=dep, engine=engine)
    for s in (0, 1, 3, 17, 63):
        alone = posterior_models(per[s], dep_int=dep, engine=engine)
        for k in ("mean", "median", "minmax", "stdminmax", "mode"):
            assert np.array_equal(a[s][k][0], alone[k][0], equal_nan=True), (s, k)
        check_site(a[s], per[s], dep, exact_cols=5)
    for s in range(S):
        for k in ("mean", "median", "minmax", "stdminmax", "mode"):
            assert np.array_equal(a[s][k][0], b[s][k][0], equal_nan=True)


def test_device_tensors_equal_the_host_path(engine):
    import torch
    from bayhunter_amd.posterior import posterior_models, posterior_hist2d
    rs = np.random.RandomState(3)
    for dt in (np.float32, np.float64):
        m = synth(rs, 4000, dtype=dt)
        m[5, 3] = np.nan                              # not a prefix: left out and counted on the device path
        site = rs.randint(0, 5, len(m)).astype(np.int32)
        mt = torch.from_numpy(m).cuda()
        st = torch.from_numpy(site).cuda()
        d = posterior_models(mt, site=st, misfits=torch.from_numpy(np.arange(len(m), 0, -1.0)), engine=engine)
        good = np.ones(len(m), bool)
        good[5] = False
        h = posterior_models(m[good], site=site[good], misfits=np.arange(len(m), 0, -1.0)[good], engine=engine)
        for s in range(5):
            assert d[s]["invalid_rows"] == (1 if s == site[5] else 0)
            for k in ("mean", "median", "minmax", "stdminmax", "mode", "minmisfit"):
                for x, y in zip(d[s][k], h[s][k]):
                    assert np.array_equal(x, y), (s, k)
        hd = posterior_hist2d(mt[good.nonzero()[0]], site=st[good.nonzero()[0]], engine=engine)
        hh = posterior_hist2d(m[good], site=site[good], engine=engine)
        for s in range(5):
            assert np.array_equal(hd[s]["counts"], hh[s]["counts"])
            assert np.array_equal(hd[s]["interfaces"], hh[s]["interfaces"])


def test_64_sites_of_50000_models(engine):
    """64 sites x 50 000 float32 models (the 200 000-model case runs in tools/gpu_posterior_perf.py): checked against the
    restatement on four sites."""
    from bayhunter_amd.posterior import posterior_models
    rs = np.random.RandomState(9)
    S, N = 64, 50000
    base = synth(rs, 4096)
    rows = base[rs.randint(0, len(base), S * N)]
    rows[:, 0] += rs.randint(-20, 20, len(rows)).astype(np.float32) * np.float32(0.001)
    site = np.repeat(np.arange(S, dtype=np.int32), N)
    r = posterior_models(rows, site=site, engine=engine)
    for s in (0, 21, 42, 63):
        check_site(r[s], rows[s * N:(s + 1) * N], np.linspace(0, 100, 201), exact_cols=3)


def test_bad_input_is_einval(engine):
    from bayhunter_amd import engine as E
    from bayhunter_amd.posterior import posterior_models, _Loaded, depth_bins
    rs = np.random.RandomState(1)
    m = synth(rs, 50, ML=4)

    def einval(fn):
        with pytest.raises(E.EngineError) as ei:
            fn()
        assert "(-1)" in str(ei.value)
    einval(lambda: posterior_models(m, dep_int=np.array([0.0, 2.0, 1.0]), engine=engine))        # unsorted grid
    bad = m.copy()
    bad[7, 1] = np.nan
    einval(lambda: posterior_models(bad, engine=engine))                                     # not a prefix (host)
    einval(lambda: posterior_models(m, site=np.full(len(m), -1, np.int32), nsites=2, engine=engine))  # site out of range
    einval(lambda: posterior_models(np.full((3, 66), np.nan), engine=engine))                    # width above 64
    wild = m.copy()
    wild[0, 0] = 1e9                                                                           # a wild vs range
    einval(lambda: posterior_models(wild, engine=engine))
    ld = _Loaded(m, None, engine)                                                              # the bound in the engine
    dep = np.linspace(0, 100, 201)
    try:
        einval(lambda: ld.hist(dep, depth_bins(dep, dep), 200, [np.linspace(2, 5, (1 << 20) + 1)]))
        c, _ = ld.hist(dep, depth_bins(dep, dep), 200, [np.linspace(2, 5, 121)])             # and the handle still works
        assert c[0].sum() == 50 * 201
    finally:
        ld.close()



def test_posterior_from_storage_summarises_every_site(tmp_path, engine):
    import bayhunter_amd as bh
    from bayhunter_amd.posterior import posterior_models
    rs = np.random.RandomState(21)
    paths, per, mis = [], [], []
    for s, ML in enumerate((21, 12, 21)):
        p = tmp_path / ("st%d" % s)
        p.mkdir()
        m = synth(rs, 500 + 50 * s, ML=ML).astype(np.float64)
        f = rs.uniform(0.1, 1, (len(m), 3))
        np.save(str(p / "c_models.npy"), m)
        np.save(str(p / "c_misfits.npy"), f)
        paths.append(str(p))
        per.append(m)
        mis.append(f[:, -1])
    got = bh.posterior_from_storage(paths, engine=engine)
    assert len(got) == 3
    for s in range(3):
        alone = posterior_models(per[s], misfits=mis[s], engine=engine)
        for k in ("mean", "median", "minmax", "stdminmax", "mode", "minmisfit"):
            for x, y in zip(got[s][k], alone[k]):
                assert np.array_equal(x, y), (s, k)
