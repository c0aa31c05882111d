"""The chain diagnostics on the GPU (include/bh_engine_chain_diag.h, bayhunter_amd/diagnostics.py): the sums of the series against
the restatement tests/diag_ref.py, each held to the bound of floating-point summation computed from its own terms; their
determinism; the model-row series against the series of a table built on the host; the refusals; the derived numbers; the
medians and outliers; and a recorded run end to end."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import diag_ref as R
from conftest import REPO, golden
import bayhunter_amd as bh
from bayhunter_amd import diagnostics as D
from bayhunter_amd import engine as E
from bayhunter_amd import results
from bayhunter_amd.chains import _is_fixed
from bayhunter_amd.device_chains import DeviceChains
from bayhunter_amd.posterior import stepmodel
from test_gpu_chains import SETUPS, make_targets
from test_gpu_sites_priors import SITE_INIT, SITE_PRIORS, full_site

pytestmark = pytest.mark.gpu

TILE, MAXLAG = E.DIAG_TILE, E.DIAG_MAXLAG
KEYS = D.FIELDS + ("p",)


def test_python_constants_mirror_the_header():
    txt = open(os.path.join(REPO, "include", "bh_engine_chain_diag.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define\s+(BH_DIAG_[A-Z]+)\s+(\d+)\b", txt, flags=re.M)}
    assert (defs["BH_DIAG_MAXLAG"], defs["BH_DIAG_MAXCOLS"], defs["BH_DIAG_MAXDEPTHS"], defs["BH_DIAG_TILE"], defs["BH_DIAG_LAGBLOCK"]) == \
        (E.DIAG_MAXLAG, E.DIAG_MAXCOLS, E.DIAG_MAXDEPTHS, E.DIAG_TILE, E.DIAG_LAGBLOCK) == (2048, 64, 63, 256, 1024)
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert sorted(set(re.findall(r"\b(bh_[a-z_]+)\s*\(", txt))) == sorted(E.CHAIN_DIAG_SYMBOLS)
    lib = C.CDLL(E.LIB_PATH)
    assert all(hasattr(lib, n) for n in E.CHAIN_DIAG_SYMBOLS) and lib.bh_abi_version() == 10


def make_table(seed, T, Cn, Q, dtype):
    """[T][C][Q]: column 0 like a likelihood series (near -1e4, unit spread), the last column of Q >= 3 constant, the rest of mixed
    scale and sign"""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((T, Cn, Q)) * (10.0 ** rs.randint(-3, 4, size=(1, Cn, Q)))
    x[:, :, 0] = -1e4 + rs.standard_normal((T, Cn))
    if Q >= 3:
        x[:, :, Q - 1] = rs.standard_normal((1, Cn)) * 100.0
    return x.astype(dtype)


def strided(x):
    """x inside a larger array of NaN: another ld_t, ld_c > Q, an offset; the gaps must never be read"""
    T, Cn, Q = x.shape
    big = np.full((2 * T + 1, Cn + 2, Q + 3), np.nan, x.dtype)
    view = big[1:2 * T + 1:2, 1:Cn + 1, 2:Q + 2]
    view[...] = x
    return big, (slice(1, 2 * T + 1, 2), slice(1, Cn + 1), slice(2, Q + 2))


def same(a, b):
    return all(np.array_equal(a[k], b[k]) and not np.any(np.signbit(a[k]) != np.signbit(b[k])) for k in KEYS) and \
        a["T"] == b["T"] and a["maxlag"] == b["maxlag"]


def check_series(x, out, L, c, q):
    """the returned sums of series (c, q) against their exact values, each within n * 2^-53 * sum |terms|"""
    T = x.shape[0]
    r1 = R.pass1(x[:, c, q])
    assert out["x0"][c, q] == r1["x0"]
    for k in ("s1", "s1a", "s1b"):
        val, bound = r1[k]
        assert abs(out[k][c, q] - val) <= bound, (k, c, q, out[k][c, q], val, bound)
    m, ma, mb = R.means(T, out["s1"][c, q], out["s1a"][c, q], out["s1b"][c, q])
    r2 = R.pass2(r1["d"], m, ma, mb, L)
    for k in ("m2a", "m2b"):
        val, bound = r2[k]
        assert abs(out[k][c, q] - val) <= bound, (k, c, q, out[k][c, q], val, bound)
    for lag, (val, bound) in enumerate(r2["p"]):
        assert abs(out["p"][c, q, lag] - val) <= bound, ("p", lag, c, q, out["p"][c, q, lag], val, bound)
    if np.all(x[:, c, q] == x[0, c, q]):
        assert all(out[k][c, q] == 0.0 for k in ("s1", "s1a", "s1b", "m2a", "m2b")) and not out["p"][c, q].any()


# T in {1, 2, 3, 7, tile-1, tile, tile+1, 2 tile + L + 3}, L in {0, 1, 63, 64, 65, T-1, T, T+5, MAXLAG with T = MAXLAG + 2},
# C in {1, 3, 65}, Q in {1, 3, 64}; the terms of the large ones (T * L of them per series) are kept to a few series
CASES = [(1, 0, 1, 1), (1, 6, 3, 3), (2, 1, 3, 3), (3, 3, 1, 3), (7, 6, 3, 1), (7, 12, 1, 3), (7, 3, 65, 64),
         (TILE - 1, 63, 3, 3), (TILE, 64, 1, 3), (TILE + 1, 65, 3, 1), (TILE + 1, 0, 1, 64), (2 * TILE + 65 + 3, 65, 1, 3),
         (2 * TILE + 1030 + 3, 1030, 1, 3), (MAXLAG + 2, MAXLAG, 1, 1)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("T,L,Cn,Q", CASES)
def test_series_sums_against_the_restatement(engine, T, L, Cn, Q, dtype):
    """A contiguous host table against the restatement, series by series; the same table as a strided host view, as a device tensor
    and as a strided device view gives the same bits."""
    import torch
    x = make_table(T * 1000 + L, T, Cn, Q, dtype)
    out = D.chain_series_stats(x, L, engine=engine)
    assert out["p"].shape == (Cn, Q, L + 1) and out["T"] == T and out["maxlag"] == L
    picks = [(c, q) for c in range(Cn) for q in range(Q)]
    if len(picks) > 64:
        rs = np.random.RandomState(1)
        picks = [(0, 0), (Cn - 1, Q - 1), (0, Q - 1), (Cn - 1, 0)] + [(rs.randint(Cn), rs.randint(Q)) for _ in range(40)]
    for c, q in picks:
        check_series(x, out, L, c, q)
    big, sl = strided(x)
    assert same(out, D.chain_series_stats(big[sl], L, engine=engine))
    dev = torch.device("cuda", 0)
    assert same(out, D.chain_series_stats(torch.from_numpy(x).to(dev), L, engine=engine))
    tbig = torch.from_numpy(big).to(dev)
    view = tbig[sl]
    assert view.data_ptr() != tbig.data_ptr() and view.shape == x.shape
    assert same(out, D.chain_series_stats(view, L, engine=engine))
    if Q == 1:     # the [T][C] form of likes and vpvs
        assert same(out, D.chain_series_stats(torch.from_numpy(x[:, :, 0].copy()).to(dev), L, engine=engine))


def test_a_series_has_the_same_bits_alone_and_among_others(engine):
    import torch
    T, L = 300, 70
    x = make_table(5, T, 65, 1, np.float32)
    dev = torch.device("cuda", 0)
    alone = D.chain_series_stats(x[:, 37:38], L, engine=engine)
    among = D.chain_series_stats(x, L, engine=engine)
    again = D.chain_series_stats(x, L, engine=engine)
    assert same(among, again)
    big, sl = strided(x)
    view = D.chain_series_stats(torch.from_numpy(big).to(dev)[sl], L, engine=engine)
    assert same(among, view) and same(view, D.chain_series_stats(torch.from_numpy(big).to(dev)[sl], L, engine=engine))
    wide = D.chain_series_stats(np.repeat(x[:, 37:38, :], 3, axis=2), L, engine=engine)     # ... and as column 1 of 3
    for k in KEYS:
        assert np.array_equal(alone[k][0, 0], among[k][37, 0]) and np.array_equal(alone[k][0, 0], wide[k][0, 1])
    # other lag limits: the sums up to the smaller one do not change
    fewer = D.chain_series_stats(x, 20, engine=engine)
    assert np.array_equal(fewer["p"], among["p"][:, :, :21]) and all(np.array_equal(fewer[k], among[k]) for k in D.FIELDS)


def model_rows(seed, T, Cn, ML, dtype):
    """rows of 1..ML layers; depths on a grid of 0.25, so the interfaces fall on multiples of 0.125"""
    rs = np.random.RandomState(seed)
    rows = np.full((T, Cn, 2 * ML), np.nan, dtype)
    for t in range(T):
        for c in range(Cn):
            n = 1 + (t * Cn + c) % ML
            z = np.sort(rs.choice(np.arange(0, 240), n, replace=False)) * 0.25
            rows[t, c, :n] = np.round(rs.uniform(2.0, 5.0, n), 3)
            rows[t, c, n:2 * n] = z
    return rows


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("ML,T,Cn,L", [(6, 37, 3, 20), (32, 70, 2, 8)])
def test_model_series_equal_the_series_of_the_host_table(engine, ML, T, Cn, L, dtype):
    import torch
    rows = model_rows(ML, T, Cn, ML, dtype)
    dep = np.concatenate((np.arange(0, 60, 1.0), [60.125, 75.5, 200.0]))
    assert dep.size == E.DIAG_MAXDEPTHS
    table = np.zeros((T, Cn, dep.size + 1))
    on_interface = 0
    for t in range(T):
        for c in range(Cn):
            vs_step, dep_step = stepmodel(rows[t, c])
            table[t, c, :-1] = np.interp(dep, dep_step, vs_step)
            table[t, c, -1] = vs_step.size // 2 - 1
            on_interface += int(np.isin(dep_step[1:-1], dep).sum())
    assert on_interface > 10 and set(table[:, :, -1].ravel()) == set(range(ML))
    want = D.chain_series_stats(table, L, engine=engine)
    got = D.chain_model_stats(rows, dep, L, engine=engine)
    assert same(want, got)
    dev = torch.device("cuda", 0)
    assert same(want, D.chain_model_stats(torch.from_numpy(rows).to(dev), dep, L, engine=engine))
    big = np.full((T + 1, Cn + 1, 2 * ML + 2), np.nan, dtype)
    big[1:, :Cn, :2 * ML] = rows
    assert same(want, D.chain_model_stats(torch.from_numpy(big).to(dev)[1:, :Cn, :2 * ML], dep, L, engine=engine))
    few = D.chain_model_stats(rows, dep[:0], L, engine=engine)          # no depths: nlayers alone
    assert all(np.array_equal(few[k][:, 0], want[k][:, -1]) for k in KEYS)


FILL = -7777.0


def raw_call(engine, x, L, Q=None, elem=None, null=None, models_dep=None):
    """bh_chain_diag_series / _models on a contiguous host table with prefilled outputs: (rc, outputs)"""
    T, Cn, W = x.shape
    Q = W if Q is None else Q
    nq = Q if models_dep is None else len(models_dep) + 1
    Lc = max(0, min(L, MAXLAG))
    outs = [np.full((Cn, nq), FILL) for _ in D.FIELDS] + [np.full((Cn, nq, Lc + 1), FILL)]
    ptrs = [None if null == i else E._ptr(o) for i, o in enumerate(outs)]
    elem = x.itemsize if elem is None else elem
    if models_dep is None:
        rc = engine._L.bh_chain_diag_series(engine._h, E.HOST, None, elem, T, Cn, Q, Cn * W, W, E._ptr(x), L, *ptrs)
    else:
        dep = np.ascontiguousarray(models_dep, np.float64)
        rc = engine._L.bh_chain_diag_models(engine._h, E.HOST, None, elem, T, Cn, W // 2, Cn * W, W, E._ptr(x), len(dep), E._ptr(dep), L,
                                            *ptrs)
    return rc, outs


def test_refusals_leave_the_outputs_untouched(engine):
    x = make_table(9, 20, 2, 3, np.float64)
    rc, outs = raw_call(engine, x, 4)
    assert rc == E.BH_OK and not any(np.any(o == FILL) for o in outs)
    wide = make_table(9, 5, 1, 65, np.float64)
    rows = model_rows(2, 6, 2, 4, np.float32)
    bad_row, odd_row, empty_row = rows.copy(), rows.copy(), rows.copy()
    bad_row[3, 1, 0] = np.nan                 # a gap before the values
    odd_row[2, 0, :] = np.nan
    odd_row[2, 0, :3] = 1.0                   # an odd count
    empty_row[5, 1, :] = np.nan               # no values at all
    inf_row = rows.copy()
    inf_row[1, 0, 0] = np.inf
    cases = []
    for v in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[13, 1, 2] = v
        cases.append(("value %r" % v, dict(x=y, L=4)))
    cases += [("Q = 65", dict(x=wide, L=2)), ("L = MAXLAG + 1", dict(x=x, L=MAXLAG + 1)), ("L < 0", dict(x=x, L=-1)),
              ("elem_bytes 2", dict(x=x, L=4, elem=2))]
    cases += [("NULL output %d" % i, dict(x=x, L=4, null=i)) for i in range(7)]
    cases += [("dep not ascending", dict(x=rows, L=2, models_dep=[0.0, 2.0, 2.0])), ("dep not finite", dict(x=rows, L=2, models_dep=[0.0, np.nan])),
              ("D = 64", dict(x=rows, L=2, models_dep=np.arange(64.0))),
              ("a gap in a row", dict(x=bad_row, L=2, models_dep=[1.0, 2.0])), ("an odd row", dict(x=odd_row, L=2, models_dep=[1.0, 2.0])),
              ("an empty row", dict(x=empty_row, L=2, models_dep=[1.0, 2.0])), ("inf in a row", dict(x=inf_row, L=2, models_dep=[1.0, 2.0]))]
    for what, kw in cases:
        rc, outs = raw_call(engine, **kw)
        assert rc == E.BH_EINVAL, what
        assert all(np.all(o == FILL) for o in outs), what
    rc, outs = raw_call(engine, rows, 2, models_dep=[1.0, 2.0])
    assert rc == E.BH_OK
    with pytest.raises(E.EngineError):
        y = x.astype(np.float32)
        y[0, 0, 0] = np.nan
        D.chain_series_stats(y, 3, engine=engine)
    with pytest.raises(E.EngineError):
        import torch
        t = torch.from_numpy(x).to(torch.device("cuda", 0))
        t[19, 1, 2] = float("inf")
        D.chain_series_stats(t, 3, engine=engine)


def test_convergence_of_the_device_tables_equals_the_restatement(engine):
    """Fixed-seed AR(1) tables whose pair sums (restatement, exact sums) stay more than 1e-6 from zero at the cut, so that the cut
    cannot depend on the last bits of the lag sums: rhat, ess and tau to rtol 1e-12, the cut equal."""
    import torch
    T, Cn, Q, L = 400, 6, 3, 60
    x = R.ar1(np.random.RandomState(424242), T, Cn, 0.7, Q)
    x[:, :, 1] = R.ar1(np.random.RandomState(7), T, Cn, 0.2)
    x[:, 4, 2] += 2.0
    site_of = [0, 0, 0, 1, 1, 1]
    exact = R.tables(x, L)
    for s in range(2):
        sel = [c for c in range(Cn) if site_of[c] == s]
        for q in range(Q):
            for chains in [sel] + [[c] for c in sel]:
                G = R.pair_sums(exact, chains, q)
                cut = next((j for j, g in enumerate(G) if not g > 0), len(G))
                assert all(abs(g) > 1e-6 for g in G[:cut + 1]), (s, q, chains)
    tab = D.chain_series_stats(torch.from_numpy(x).to(torch.device("cuda", 0)), L, engine=engine)
    got = D.convergence(tab, site_of)
    for s in range(2):
        chains = [c for c in range(Cn) if site_of[c] == s]
        for q in range(Q):
            r = R.convergence(tab, chains, q)
            g = got[s]
            for k in ("rhat", "ess", "tau"):
                assert abs(g[k][q] - r[k]) <= 1e-12 * abs(r[k]), (k, s, q)
            assert g["cut"][q] == r["cut"] and bool(g["ess_truncated"][q]) == r["truncated"] and not g["constant"][q]
            for j in range(len(chains)):
                for k in ("mean", "std", "chain_tau"):
                    assert abs(g[k][j, q] - r[k][j]) <= 1e-12 * abs(r[k][j]), (k, s, q, j)
    assert got[1]["rhat"][2] > got[0]["rhat"][2]          # the shifted chain of site 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("T", [1, 2, 3, 100, 1001])
def test_medians_are_numpys_bits(engine, T, dtype):
    import torch
    rs = np.random.RandomState(T)
    x = (rs.standard_normal((T, 9)) * 10.0 ** rs.randint(-2, 3, size=(1, 9))).astype(dtype)
    x[:, 1] = np.round(x[:, 1])                 # ties
    x[:, 2] = -np.abs(x[:, 2]) - 1e4            # all negative
    x[:, 3] = 2.5                               # constant
    want = np.median(x, axis=0)
    assert want.dtype == dtype
    dev = torch.device("cuda", 0)
    got = D.chain_medians(torch.from_numpy(x).to(dev), engine=engine)
    assert got.dtype == dtype and np.array_equal(got, want)
    big = np.full((T + 2, 12), np.nan, dtype)
    big[1:T + 1, 2:11] = x
    assert np.array_equal(D.chain_medians(torch.from_numpy(big).to(dev)[1:T + 1, 2:11], engine=engine), want)
    with pytest.raises(E.EngineError):
        D.chain_medians(torch.from_numpy(big).to(dev)[:, 2:11], engine=engine)


@pytest.mark.parametrize("branch", ["positive", "negative", "zero"])
@pytest.mark.parametrize("T", [100, 101])
def test_synthetic_outliers_on_the_device(engine, branch, T):
    """one chain's median pushed past dev, in each sign branch: that chain and no other"""
    import torch
    rs = np.random.RandomState(T)
    base = {"positive": 2000.0, "negative": -2000.0, "zero": 0.0}[branch]
    likes = (base + rs.standard_normal((T, 8))).astype(np.float32)
    if branch == "zero":      # medians 0; the pushed chain's -50: the rule scores every chain of a site whose best median is 0 as 1
        likes = np.where(rs.uniform(size=(T, 8)) < 0.3, -1.0, 0.0).astype(np.float32)
        likes[:, 5] -= np.float32(50.0)
    site_of = np.repeat(np.arange(2), 4)
    if branch != "zero":
        likes[:, 5] -= np.float32(0.06 * 2000.0) * (1.0 if branch == "positive" else 1.1)
        likes[:, 2] -= np.float32(0.04 * 2000.0)         # within dev
    want, wscores = D.outlier_chains(likes, site_of)
    got, gscores = D.outlier_chains(torch.from_numpy(likes).to(torch.device("cuda", 0)), site_of, engine=engine)
    assert [list(o) for o in got] == [list(o) for o in want] == ([[], [5]] if branch != "zero" else [[], []])
    assert all(np.array_equal(a, b) for a, b in zip(gscores, wscores))


# ---- a recorded run end to end ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def site_run(tmp_path_factory):
    """2 sites x 4 chains under their own priors, recorded on the device (the set-up of tests/test_gpu_chain_record.py::site_runs)"""
    g = golden("chain_golden.npz")
    root = tmp_path_factory.mktemp("diag_sites")
    st = bh.SiteTargets([full_site(g, s, "phase_rf") for s in range(2)], names=["st0", "st1"], per_site_x="all", per_site_rf=True)
    inits = [dict(SITE_INIT[s], savepath=str(root)) for s in range(2)]
    return DeviceChains(st, 4, inits, SITE_PRIORS[:2], seed=77, search="fast", record="device").run()


def same_result(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        if isinstance(a[k], dict):
            same_result(a[k], b[k], what + (k,))
        else:
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert x.shape == y.shape and np.array_equal(x, y, equal_nan=(x.dtype.kind == "f")), what + (k,)


def test_diagnostics_of_a_recorded_run(site_run):
    dev = site_run
    diag = dev.diagnostics()
    assert len(diag) == 2
    h = dev.samples("p2")
    T = h["likes"].shape[0]
    assert T >= 4 and diag[0]["maxlag"] == min(T // 2, 1000) and np.array_equal(diag[0]["dep"], np.linspace(0, 100, 41))
    # the same calls on the host arrays: the same kernels on the same values
    host = D.diagnose(h, np.arange(8) // 4, np.arange(8), engine=dev.engine)
    folders = dev.save()
    stored = results.diagnostics_from_storage(folders, engine=dev.engine)
    nt = dev.nt
    for s in range(2):
        same_result(diag[s], host[s], (s, "host"))
        d, f = diag[s], stored[s]
        assert np.array_equal(d["outliers"], f["outliers"]) and np.array_equal(d["scores"], f["scores"])
        assert np.array_equal(d["outliers"], results.get_outliers(folders[s]).astype(np.int64))
        for k in ("likes", "vpvs", "misfits", "noise", "nlayers", "vs"):       # (no site lacks a target: the same columns)
            same_result(d[k], f[k], (s, "stored", k))
        for k, width in (("likes", 1), ("vpvs", 1), ("misfits", nt + 1), ("noise", 2 * nt), ("vs", 41)):
            assert d[k]["rhat"].shape == (width,) and d[k]["mean"].shape == (len(d[k]["chains"]), width)
        assert d["nlayers"]["rhat"].shape == () and set(d["likes"]["chains"]) == set(range(4 * s, 4 * s + 4)) - set(d["outliers"])
        fixed = np.array([_is_fixed(p) or p[0] == p[1] for p in dev.site_noisepriors[s]])
        assert fixed.any() and np.all(d["noise"]["constant"][fixed])       # a fixed parameter is flagged ...
        for k in ("noise", "misfits", "vpvs", "likes"):                   # ... and so is, exactly, every column no kept chain moves in
            cols = h[k][:, d[k]["chains"]].reshape(T, len(d[k]["chains"]), -1)
            assert np.array_equal(d[k]["constant"], np.all(cols == cols[:1], axis=(0, 1))), (s, k)
            c = d[k]["constant"]
            assert np.all(np.isnan(d[k]["rhat"][c])) and np.all(np.isnan(d[k]["ess"][c])) and np.all(np.isfinite(d[k]["rhat"][~c]))
            assert np.all(d[k]["ess"][~c] > 0)
        assert not d["likes"]["constant"][0] and not d["misfits"]["constant"][-1]
        if _is_fixed(dev.site_priors[s]["vpvs"]):
            assert d["vpvs"]["constant"][0]
    outl = np.concatenate([d["outliers"] for d in diag])
    ps = dev.posterior_scalars(exclude_chains=outl)
    assert len(ps) == 2
    # a sequence overrides the outliers
    over = dev.diagnostics(exclude_chains=[1, 6], maxlag=5, dep=[1.0, 30.0])
    assert list(over[0]["likes"]["chains"]) == [0, 2, 3] and list(over[1]["vs"]["chains"]) == [4, 5, 7]
    assert over[0]["vs"]["rhat"].shape == (2,) and over[1]["maxlag"] == 5 and np.array_equal(over[0]["outliers"], diag[0]["outliers"])


def test_diagnostics_refuses_host_records_and_tempered_runs():
    g = golden("chain_golden.npz")
    su = SETUPS["exp"]
    init = dict(su["init"], iter_burnin=280, iter_main=60, maxmodels=15)
    host = DeviceChains(make_targets(g), 4, init, su["priors"], seed=5, record="host")
    with pytest.raises(E.EngineError, match="record='device'"):
        host.diagnostics()
    ladder = np.repeat(np.arange(2), 4)
    betas = np.tile(1.0 / np.geomspace(1.0, 20.0, 4), 2)
    tempered = DeviceChains(make_targets(g), 8, init, su["priors"], seed=5, betas=betas, ladder=ladder, swap_every=20, record="device")
    with pytest.raises(E.EngineError, match="tempered"):
        tempered.diagnostics()
