"""GPU tests of the feature series of the chains (include/bh_engine_chain_diag_features.h; bayhunter_amd/diagnostics.py:
chain_feature_series, feature_convergence, diagnose(features=, moho=)): the kernel against the restatement tests/features_ref.py and
against the columns bh_posterior_features forms for the same rows, bit for bit; gathered series; refusals that write nothing; and
recorded runs end to end."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import feature_series_ref as FS
from conftest import REPO
from bayhunter_amd import diagnostics as D
from bayhunter_amd import engine as E
from bayhunter_amd import results
from bayhunter_amd.posterior import check_features, posterior_classes
from test_gpu_chain_diag import same_result, site_run                      # noqa: F401  (the recorded run of the diagnostics tests)
from test_gpu_chain_diag_ladders import tempered_run                       # noqa: F401
from test_gpu_posterior_features import make_rows

pytestmark = pytest.mark.gpu

FILL = -7.25
SITE6 = np.array([0, 0, 0, 1, 1, 1])          # 6 chains over 2 sites: a wavefront straddles the change of the parameters
# one feature of every kind; the two sites' windows and thresholds differ
NINE = {"mean": ("vsmean", [5.0, 0.0], [30.0, 45.25]), "time": ("vstime", [0.0, 2.0], [30.0, 9.0]), "tts": ("tts", 0.0, [3.0, 4.0]),
        "slow": ("vsmin", [6.0, 1.0], [40.0, 55.25]), "fast": ("vsmax", [6.0, 1.0], [40.0, 55.25]),
        "lvz": ("drop", [5.0, 0.0], [30.0, 45.25], [0.5, 0.75]), "step": ("jump", [5.0, 0.0], [30.0, 45.25], [0.4, 0.8]),
        "moho": ("above", [5.0, 0.0], [30.0, 45.25], [3.4, 3.2]), "nif": ("nifaces", [0.0, 0.25], [20.0, 25.0])}
ONE = {"sed": ("above", [0.0, 1.0], [12.0, 20.0], [2.5, 3.0])}
# 32 kinds of two columns: exactly BH_SCALARS_MAXCOLS columns
WIDE = {"f%02d" % i: (("vsmin", "vsmax", "drop", "jump")[i % 4], [0.5 * i, 0.25 * i], [20.0 + i, 30.0 + 2 * i]) + (([0.1 * (i % 5), 0.3],) if i % 4 >= 2 else ())
        for i in range(32)}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def host(a):
    return a.cpu().numpy() if D._is_tensor(a) else np.asarray(a)


def place(x, memspace):
    if memspace == "host":
        return x
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))


def strided(x, memspace):
    """the table as a view with ld_c > 2*ML and ld_t > C * ld_c"""
    T, Cn, W = x.shape
    big = np.full((T, Cn + 2, W + 3), 1e30, x.dtype)
    big[:, 1:Cn + 1, :W] = x
    return place(big, memspace)[:, 1:Cn + 1, :W]


_TABLES = {}


def table(T, ML, dtype):
    """(models [T][6][2*ML], the reference's value, present, missing for NINE), built once"""
    key = (T, ML, np.dtype(dtype).str)
    if key not in _TABLES:
        rs = np.random.RandomState(100 * T + ML)
        rows = make_rows(rs, T * 6, ML, dtype, "a" if dtype == np.float64 else "b").reshape(T, 6, 2 * ML)
        kinds, par, labels = check_features(NINE, 2)
        _TABLES[key] = (rows,) + FS.series_ref(rows, kinds, par, SITE6)
    return _TABLES[key]


def test_python_constants_mirror_the_header():
    txt = open(os.path.join(REPO, "include", "bh_engine_chain_diag_features.h")).read()
    assert sorted(set(re.findall(r"\b(bh_[a-z_]+)\s*\(", txt))) == sorted(E.CHAIN_DIAG_FEATURES_SYMBOLS)
    lib = E.load_library()
    assert all(hasattr(lib, n) for n in E.CHAIN_DIAG_FEATURES_SYMBOLS) and lib.bh_abi_version() == 10


def class_columns(rows, features, engine):
    """the columns bh_posterior_features forms for the same rows, by input row: label -> float64 [T][6]"""
    T = rows.shape[0]
    got = posterior_classes(rows.reshape(T * 6, -1), {"all": []}, site=np.tile(SITE6, T).astype(np.int32), features=features,
                            engine=engine, nsites=2, return_columns=True)
    assert np.all(got["cls"] == 0)
    return {k: v.reshape(T, 6) for k, v in got["columns"].items()}


@pytest.mark.parametrize("memspace", ["host", "device"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("ML", [1, 5])
@pytest.mark.parametrize("T", [1, 37, 130])
def test_the_series_are_the_restatements_and_the_posterior_columns(engine, T, ML, dtype, memspace):
    rows, value, present, missing = table(T, ML, dtype)
    x = place(rows, memspace)
    v, p, m, labels = D.chain_feature_series(x, NINE, SITE6, engine=engine)
    assert D._is_tensor(v) == (memspace == "device") and D._is_tensor(p) == (memspace == "device") and len(labels) == 13
    assert host(v).dtype == np.float64 and host(p).dtype == np.float32 and m.dtype == np.int64
    assert same_bits(host(v), value) and same_bits(host(p), present) and np.array_equal(m, missing)
    if ML == 5 and T >= 37:      # the optional kinds are there in some rows and lacking in others, at both sites
        for q in (labels.index("lvz.depth"), labels.index("step.depth"), labels.index("moho")):
            for s in range(2):
                assert 0 < present[:, SITE6 == s, q].mean() < 1, (labels[q], s)
    # the columns of the loaded handle for the same rows
    cols = class_columns(rows, NINE, engine)
    for q, lb in enumerate(labels):
        assert same_bits(present[:, :, q], (~np.isnan(cols[lb])).astype(np.float32)), lb
        assert same_bits(value[:, :, q], np.where(np.isnan(cols[lb]), 0.0, cols[lb])), lb
    # a strided view; on a repeat; a series alone
    v2, p2, m2, _ = D.chain_feature_series(strided(rows, memspace), NINE, SITE6, engine=engine)
    assert same_bits(host(v2), value) and same_bits(host(p2), present) and np.array_equal(m2, missing)
    v3, p3, m3, _ = D.chain_feature_series(x, NINE, SITE6, engine=engine)
    assert same_bits(host(v3), value) and same_bits(host(p3), present) and np.array_equal(m3, missing)
    v1, p1, m1, _ = D.chain_feature_series(x[:, 4:5], NINE, [1], engine=engine, nsites=2)
    assert same_bits(host(v1), value[:, 4:5]) and same_bits(host(p1), present[:, 4:5]) and np.array_equal(m1, missing[4:5])


def raw(engine, x, site, kinds, par, memspace="host", sel=None, K=None, nsites=2, elem=None, ld_out=None, F=None, null=(), ld_sel=None):
    """bh_chain_diag_features on a contiguous table x [T][C][2*ML] with prefilled outputs: (rc, value, present, missing) -- the outputs
    with the leading dimensions ld_out = (ld_out_t, ld_out_k) as flat buffers, FILL where nothing was written"""
    T, Cn, W = x.shape
    kinds = None if kinds is None else np.ascontiguousarray(kinds, np.int32)
    par = None if par is None else np.ascontiguousarray(par, np.float64)
    F = (0 if kinds is None else len(kinds)) if F is None else F
    ncols = 0 if kinds is None else int(sum(2 if 3 <= k <= 6 else 1 for k in kinds))
    Kn = (Cn if sel is None else sel.shape[1]) if K is None else K
    ld_t, ld_k = (Kn * max(ncols, 1), max(ncols, 1)) if ld_out is None else ld_out
    n = max(1, (T - 1) * ld_t + (max(Kn, 1) - 1) * ld_k + max(ncols, 1))
    site = np.ascontiguousarray(site, np.int32)
    missing = np.full((max(Kn, 1), max(ncols, 1)), -1, np.int64)
    xs, ss = place(x, memspace), (None if sel is None else place(np.ascontiguousarray(sel, np.int32), memspace))
    value, present = place(np.full(n, FILL), memspace), place(np.full(n, FILL, np.float32), memspace)
    if memspace == "host":
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        mem = E.HOST
    else:
        ptr = lambda a: None if a is None else C.c_void_p(a.data_ptr())
        mem = E.DEVICE
    rc = engine._L.bh_chain_diag_features(
        engine._h, mem, None, x.itemsize if elem is None else elem, T, Cn, W // 2, Cn * W, W, None if "models" in null else ptr(xs), Kn,
        ptr(ss), (Kn if ld_sel is None else ld_sel), nsites, None if "site" in null else E._ptr(site), F,
        None if kinds is None else E._ptr(kinds), None if par is None else E._ptr(par), None if "value" in null else ptr(value),
        None if "present" in null else ptr(present), ld_t, ld_k, None if "missing" in null else E._ptr(missing))
    if memspace == "device":
        import torch
        torch.cuda.synchronize()
    return rc, host(value), host(present), missing


def untouched(value, present, missing):
    return np.all(value == FILL) and np.all(present == FILL) and np.all(missing == -1)


@pytest.mark.parametrize("memspace", ["host", "device"])
@pytest.mark.parametrize("features", [ONE, WIDE], ids=["one", "wide"])
def test_one_column_and_exactly_64_columns_with_any_leading_dimensions(engine, features, memspace):
    rows = table(37, 5, np.float32)[0]
    kinds, par, labels = check_features(features, 2)
    Q = len(labels)
    assert Q == (1 if features is ONE else E.SCALARS_MAXCOLS)
    value, present, missing = FS.series_ref(rows, kinds, par, SITE6)
    v, p, m, _ = D.chain_feature_series(place(rows, memspace), features, SITE6, engine=engine)
    assert same_bits(host(v), value) and same_bits(host(p), present) and np.array_equal(m, missing)
    # outputs whose series and rows lie further apart: the same bits where they belong, nothing in between
    ld_k, ld_t = Q + 2, 6 * (Q + 2) + 5
    rc, fv, fp, fm = raw(engine, rows, SITE6, kinds, par, memspace, ld_out=(ld_t, ld_k))
    assert rc == E.BH_OK and np.array_equal(fm, missing)
    at = (np.arange(37)[:, None, None] * ld_t + np.arange(6)[None, :, None] * ld_k + np.arange(Q)[None, None, :]).reshape(-1)
    assert same_bits(fv[at].reshape(37, 6, Q), value) and same_bits(fp[at].reshape(37, 6, Q), present)
    gap = np.ones(fv.size, bool)
    gap[at] = False
    assert np.all(fv[gap] == FILL) and np.all(fp[gap] == FILL)


def selection(T):
    """K = 2 series over the 6 chains, the chain of each changing every 5 rows within its site"""
    t = np.arange(T)
    return np.stack([(t // 5) % 3, 3 + (t // 5 + 1) % 3], axis=1).astype(np.int32)


@pytest.mark.parametrize("memspace", ["host", "device"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_gathered_series_read_the_selected_chain_and_nothing_else(engine, dtype, memspace):
    T = 37
    rows = table(T, 5, dtype)[0]
    sel = selection(T)
    assert len(np.unique(sel[:, 0])) == 3 and np.any(np.diff(sel[:, 1]) != 0)
    kinds, par, _ = check_features(NINE, 2)
    picked = np.take_along_axis(rows, sel.astype(np.int64)[:, :, None], 1)
    want = D.chain_feature_series(place(picked, memspace), NINE, [0, 1], engine=engine)
    ref = FS.series_ref(rows, kinds, par, [0, 1], sel=sel)
    assert same_bits(host(want[0]), ref[0]) and same_bits(host(want[1]), ref[1]) and np.array_equal(want[2], ref[2])
    # rows of chains not selected at a row are poison: NaN throughout, a gap, an infinity
    poison = rows.copy()
    for t in range(T):
        for c in range(6):
            if c not in sel[t]:
                poison[t, c] = (np.nan, np.inf, 1.0)[(t + c) % 3]
                poison[t, c, 1] = np.nan
    for s in (place(sel, memspace), place(np.concatenate([sel, sel + 99], axis=1), memspace)[:, :2]):      # ... and ld_sel > K
        got = D.chain_feature_series(place(poison, memspace), NINE, [0, 1], sel=s, engine=engine)
        assert same_bits(host(got[0]), host(want[0])) and same_bits(host(got[1]), host(want[1])) and np.array_equal(got[2], want[2])
    assert D._is_tensor(got[0]) == (memspace == "device")


@pytest.mark.parametrize("memspace", ["host", "device"])
def test_refusals_write_nothing(engine, memspace):
    rows = table(37, 5, np.float64)[0].copy()
    kinds, par, _ = check_features(NINE, 2)
    sel = selection(37)
    rc, v, p, m = raw(engine, rows, SITE6, kinds, par, memspace)
    assert rc == E.BH_OK and not np.any(v == FILL) and not np.any(p == FILL) and not np.any(m == -1)
    rc, v, p, m = raw(engine, rows, [0, 1], kinds, par, memspace, sel=sel)
    assert rc == E.BH_OK and not np.any(v == FILL)

    def data(t, c, i, val):
        y = rows.copy()
        y[t, c, i] = val
        return y

    odd = rows.copy()
    odd[20, 2] = np.nan
    odd[20, 2, :3] = 1.0
    empty = rows.copy()
    empty[36, 5] = np.nan
    two = ("vsmin",) * 33
    cases = [("index == C", dict(x=rows, site=[0, 1], sel=np.where(np.arange(74).reshape(37, 2) == 41, 6, sel), match="index")),
             ("index < 0", dict(x=rows, site=[0, 1], sel=np.where(np.arange(74).reshape(37, 2) == 0, -1, sel), match="index")),
             ("an infinite vs", dict(x=data(7, 3, 0, np.inf), match="finite")),
             ("-inf in a depth", dict(x=data(36, 5, 1, -np.inf), match="finite")),
             ("a gap in a row", dict(x=data(11, 0, 0, np.nan), match="prefix")),
             ("an odd row", dict(x=odd, match="prefix")), ("an empty row", dict(x=empty, match="prefix")),
             ("a site beyond nsites", dict(site=[0, 0, 0, 1, 1, 2], match="site")), ("a negative site", dict(site=[0, 0, -1, 1, 1, 1], match="site")),
             ("nsites 0", dict(nsites=0, match="nsites")),
             ("F = 0", dict(F=0, match="F")), ("F = 65", dict(F=65, match="F")),
             ("kind NULL", dict(kinds=None, F=9, match="null")), ("par NULL", dict(par=None, match="null")),
             ("no such kind", dict(kinds=np.where(np.arange(9) == 4, 9, kinds), match=r"kind\[4\]")),
             ("a negative kind", dict(kinds=np.where(np.arange(9) == 0, -1, kinds), match=r"kind\[0\]")),
             ("65 columns", dict(kinds=[3] * 32 + [0], par=np.tile([0.0, 10.0, 0.0], (2, 33, 1)), match="BH_SCALARS_MAXCOLS")),
             ("elem_bytes 2", dict(elem=2, match="float32")), ("K != C without sel", dict(K=5, site=[0, 0, 0, 1, 1], match="K")),
             ("ld_out_k < columns", dict(ld_out=(6 * 13, 12), match="leading")), ("ld_sel < K", dict(site=[0, 1], sel=sel, ld_sel=1, match="ld_sel")),
             ("models NULL", dict(null=("models",), match="null")), ("site NULL", dict(null=("site",), match="null")),
             ("value NULL", dict(null=("value",), match="null")), ("present NULL", dict(null=("present",), match="null")),
             ("missing NULL", dict(null=("missing",), match="null"))]
    for what, i, val, match in (("z0 not finite", 0, np.nan, "finite"), ("c infinite", 2, np.inf, "finite"), ("z0 < 0", 0, -0.5, "z0"),
                                ("z1 == z0", 1, None, "z0 < z1")):
        bad = par.copy()
        bad[1, 3, i] = bad[1, 3, 0] if val is None else val
        cases.append((what, dict(par=bad, match=r"par\[1\]\[3\]")))
    for f, what in ((5, "a negative c of a drop"), (6, "a negative c of a jump")):
        bad = par.copy()
        bad[0, f, 2] = -0.25
        cases.append((what, dict(par=bad, match=r"par\[0\]\[%d\].*negative" % f)))
    del two
    for what, kw in cases:
        match = kw.pop("match")
        args = dict(x=rows, site=SITE6, kinds=kinds, par=par)
        args.update(kw)
        rc, v, p, m = raw(engine, memspace=memspace, **args)
        assert rc == E.BH_EINVAL, what
        assert untouched(v, p, m), what
        assert re.search(match, engine._L.bh_engine_last_error(engine._h).decode()), (what, engine._L.bh_engine_last_error(engine._h))
    # ... and through Python: the errors of check_features, and the engine's
    with pytest.raises(ValueError, match="unknown kind"):
        D.chain_feature_series(rows, {"a": ("nope", 0.0, 1.0)}, SITE6, engine=engine)
    with pytest.raises(ValueError, match="needs c"):
        D.chain_feature_series(rows, {"a": ("above", 0.0, 1.0)}, SITE6, engine=engine)
    with pytest.raises(E.EngineError, match="prefix"):
        D.chain_feature_series(place(odd, memspace), NINE, SITE6, engine=engine)
    rc, v, p, m = raw(engine, rows, SITE6, kinds, par, memspace)          # the engine is as usable as before
    assert rc == E.BH_OK and not np.any(v == FILL)


# ---- recorded runs end to end -----------------------------------------------------------------------------------------------------
# `above` at rising velocities over the whole model: from nearly every row to nearly none, so that some column is there in part of a
# site's rows; a per-site number (sed's z1); kinds that no row lacks (vs30, nif)
RUN_FEATURES = {"sed": ("above", 0.0, [10.0, 12.0], 3.0), "vs30": ("vstime", 0.0, 30.0), "lvz": ("drop", 0.0, 60.0, 0.1),
                "lvz3": ("drop", 0.0, 60.0, 0.3), "a30": ("above", 0.0, 80.0, 3.0), "a34": ("above", 0.0, 80.0, 3.4),
                "a38": ("above", 0.0, 80.0, 3.8), "a42": ("above", 0.0, 80.0, 4.2), "a46": ("above", 0.0, 80.0, 4.6),
                "nif": ("nifaces", 0.0, 60.0)}
MOHO = (20.0, 50.0)
TODAY = {"outliers", "scores", "chain_ids", "dep", "maxlag"} | set(D.GROUPS)


def restated(tabs, site_of, ids, d, engine, L):
    """the "features" dict of one site from chain_series_stats on numpy-built tables (tests/feature_series_ref.py)"""
    value, present, missing = tabs
    f = d["features"]
    idx = np.flatnonzero(np.isin(ids, f["chains"]))
    assert np.array_equal(ids[idx], f["chains"]) and np.all(site_of[idx] == site_of[idx[0]])
    T = value.shape[0]
    tv, tp = D.chain_series_stats(value, 0, engine=engine), D.chain_series_stats(present, L, engine=engine)
    rule = FS.missing_rule(value, present, missing, idx, tv["x0"] + tv["s1"] / T, tp["x0"] + tp["s1"] / T)
    tx = D.chain_series_stats(np.ascontiguousarray(rule["x"]), L, engine=engine)
    zero = np.zeros(len(idx), int)
    cx, cp = D.convergence(tx, zero)[0], D.convergence(tp, np.where(np.isin(np.arange(len(ids)), idx), 0, 1))[0]
    assert np.array_equal(f["missing"], missing[idx]) and np.array_equal(f["complete"], rule["complete"])
    assert np.array_equal(f["probability"], rule["probability"]) and np.array_equal(f["mean"], rule["m"], equal_nan=True)
    for k in ("rhat", "ess", "tau", "cut", "ess_truncated", "constant", "chain_tau"):
        assert np.array_equal(f[k], cx[k], equal_nan=True), k
        assert np.array_equal(f["presence"][k], cp[k], equal_nan=True), ("presence", k)
    with np.errstate(all="ignore"):
        pq = np.where(rule["complete"], 1.0, rule["probability"])
        assert np.array_equal(f["mcse_mean"], FS.pooled_sd(tx, np.arange(len(idx))) / (pq * np.sqrt(cx["ess"])), equal_nan=True)
        assert np.array_equal(f["presence"]["mcse_probability"], FS.pooled_sd(tp, idx) / np.sqrt(cp["ess"]), equal_nan=True)
    return rule


def test_features_of_a_recorded_run(site_run):
    dev = site_run
    plain = dev.diagnostics()
    assert all(set(d) == TODAY for d in plain)                        # without features= the dicts are today's
    diag = dev.diagnostics(features=RUN_FEATURES, moho=MOHO)
    assert all(set(d) == TODAY | {"features"} for d in diag)
    for s in range(2):
        same_result({k: v for k, v in diag[s].items() if k != "features"}, plain[s], (s, "the rest"))
    h = dev.samples("p2")
    T = h["likes"].shape[0]
    L = diag[0]["maxlag"]
    site_of, ids = np.arange(8) // 4, np.arange(8)
    on_host = D.diagnose(h, site_of, ids, engine=dev.engine, features=RUN_FEATURES, moho=MOHO)
    stored = results.diagnostics_from_storage(dev.save(), engine=dev.engine, features=RUN_FEATURES, moho=MOHO)
    fts = D.moho_feature(RUN_FEATURES, MOHO, 4.2, 2)
    kinds, par, labels = check_features(fts, 2)
    assert labels[-1] == "moho" and labels[1] == "vs30" and par[1, 0, 1] == 12.0
    tabs = FS.series_ref(h["models"], kinds, par, site_of)
    v, p, m, lb = D.chain_feature_series(dev.samples_dev("p2")["models"], fts, site_of, engine=dev.engine)
    assert lb == labels and same_bits(host(v), tabs[0]) and same_bits(host(p), tabs[1]) and np.array_equal(m, tabs[2])
    # the "moho" column is posterior_moho's depth column for the same rows
    rows2d = np.ascontiguousarray(h["models"]).reshape(T * 8, -1)
    pm = posterior_classes(rows2d, {"all": []}, site=np.tile(site_of, T).astype(np.int32), moho=MOHO, engine=dev.engine, nsites=2,
                           return_columns=True)["columns"]["moho"].reshape(T, 8)
    assert same_bits(tabs[1][:, :, -1], (~np.isnan(pm)).astype(np.float32)) and same_bits(tabs[0][:, :, -1], np.where(np.isnan(pm), 0.0, pm))
    partial = complete = False
    for s in range(2):
        f = diag[s]["features"]
        assert f["labels"] == labels and set(f["chains"]) == set(range(4 * s, 4 * s + 4)) - set(diag[s]["outliers"])
        same_result(f, on_host[s]["features"], (s, "host"))
        same_result(f, stored[s]["features"], (s, "stored"))
        rule = restated(tabs, site_of, ids, diag[s], dev.engine, L)
        print("site", s, {lb: (round(float(pr), 3), round(float(e), 1), float(c)) for lb, pr, e, c in zip(labels, f["probability"], f["ess"], f["mcse_mean"])})
        partial = partial or bool(np.any((f["probability"] > 0) & (f["probability"] < 1)))
        complete = complete or bool(f["complete"][labels.index("vs30")])
        assert np.all(f["presence"]["constant"][f["complete"]]) and np.all(np.isnan(f["presence"]["mcse_probability"][f["complete"]]))
        ok = ~f["constant"]
        assert np.all(np.isfinite(f["rhat"][ok])) and np.all(f["ess"][ok] > 0) and np.all(f["mcse_mean"][ok & (f["probability"] > 0)] > 0)
        assert rule["x"].shape[1] == len(f["chains"])
    assert partial and complete                 # a feature that part of a site's rows lack, and one that no row lacks
    # rank=True: the ranks of the value table where the column is complete, of the indicator under `presence`
    ranked = dev.diagnostics(features=RUN_FEATURES, moho=MOHO, rank=True)
    for s in range(2):
        f = ranked[s]["features"]
        same_result({k: v for k, v in f.items() if k != "rank" and k != "presence"}, {k: v for k, v in diag[s]["features"].items() if k != "presence"},
                    (s, "ranked"))
        assert sorted(f["rank"]) == sorted(("chains",) + D.RANK_FIELDS) and sorted(f["presence"]["rank"]) == sorted(f["rank"])
        exclude = np.flatnonzero(~np.isin(ids, np.concatenate([ranked[i]["features"]["chains"] for i in range(2)])))
        want = D.rank_convergence(v, site_of, L, exclude, engine=dev.engine)[s]
        c = f["complete"]
        assert c.any() and np.array_equal(f["rank"]["chains"], f["chains"])
        for k in D.RANK_FIELDS:
            assert np.array_equal(f["rank"][k][c], want[k][c], equal_nan=True), k
            assert not np.any(f["rank"][k][~c]) if want[k].dtype == bool else np.all(np.isnan(f["rank"][k][~c])), k
        assert np.all(np.isfinite(f["rank"]["rhat"][c & ~f["constant"]]))


def test_features_of_a_tempered_run(tempered_run):
    dev = tempered_run
    feats = {k: RUN_FEATURES[k] for k in ("vs30", "lvz", "a38", "nif")}
    diag = dev.ladder_diagnostics(features=feats, moho=MOHO)
    h = dev.samples("p2", cold_only=True)
    want = D.diagnose(h, np.zeros(2, int), h["ladder"], engine=dev.engine, features=feats, moho=MOHO)[0]
    same_result(diag["features"], want["features"], ("cold",))
    assert diag["features"]["labels"] == ["vs30", "lvz.depth", "lvz.jump", "a38", "nif", "moho"]
    assert set(diag["features"]["chains"]) == {0, 1} - set(diag["outliers"])
    assert "features" not in dev.ladder_diagnostics()
    with pytest.raises(ValueError, match="rank"):
        dev.ladder_diagnostics(features=feats, rank=True)
    with pytest.raises(ValueError, match="rank"):
        D.diagnose(h, np.zeros(2, int), h["ladder"], engine=dev.engine, features=feats, rank=True, sel=np.zeros((h["likes"].shape[0], 2), np.int32))
