"""The rows of every site split into classes by a rule over their scalar columns, on the GPU (include/bh_engine_posterior_classes.h,
bayhunter_amd/posterior.py: posterior_classes and classes=) against the restatement tests/classes_ref.py over the columns of
tests/features_ref.py and tests/moho_ref.py: cls and counts bit for bit; the exported columns; conditioning as subsetting for the
six functions that take classes=; the refusals; a recorded run."""
import ctypes as C
import re

import numpy as np
import pytest

import classes_ref as CR
import features_ref as FR
import moho_ref as MR
from conftest import REPO
from test_gpu_chain_diag import site_run  # noqa: F401  (the recorded run's fixture)
from test_gpu_posterior_features import make_rows
from test_gpu_posterior_quantiles import same

pytestmark = pytest.mark.gpu

S3 = 3
INF = np.inf
FEATS = dict(lvz=("drop", 0.0, 60.0, [0.5, 0.75, 1.0]), crust=("vsmean", 0.0, [20.0, 25.0, 30.0]), n40=("nifaces", 0.0, 40.0))
FLABELS = ["lvz.depth", "lvz.jump", "crust", "n40"]
MOHO = np.array([[5.0, 50.0], [10.0, 45.0], [0.0, 55.0]])
MOHOVS = np.array([3.5, 3.75, 3.25])
ULABELS = ["vpvs", "noise[0]", "noise[1]", "nlayers"]
ROWS = (1, 63, 64, 65, 255, 256, 257, 1000)


def test_the_constants_and_symbols_mirror_the_header():
    from bayhunter_amd import engine as E
    txt = open(REPO + "/include/bh_engine_posterior_classes.h").read()
    defs = {k: int(v) for k, v in re.findall(r"^#define\s+(BH_[A-Z0-9_]+)\s+(-?\d+)\b", txt, flags=re.M)}
    assert defs == dict(BH_CLASSES_MAX=E.CLASSES_MAX, BH_CLASS_MAXTERMS=E.CLASS_MAXTERMS, BH_CLASS_IN=E.CLASS_IN, BH_CLASS_HAS=E.CLASS_HAS,
                        BH_CLASS_LACKS=E.CLASS_LACKS)
    body = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert sorted(set(re.findall(r"\b(bh_[a-z_0-9]+)\s*\(", body))) == sorted(E.POSTERIOR_CLASSES_SYMBOLS)
    lib = C.CDLL(E.LIB_PATH)
    assert all(hasattr(lib, n) for n in E.POSTERIOR_CLASSES_SYMBOLS) and lib.bh_abi_version() == 10


# ---- the cases: rows, what is attached to them, and the restated columns -------------------------------------------------------

_CASES = {}


def feature_par():
    from bayhunter_amd.posterior import check_features
    kinds, par, labels = check_features(FEATS, S3)
    assert labels == FLABELS
    return kinds, par


def columns_ref(rows, site, vpvs, noise):
    """label -> float64 [N]: the restated columns of all three sets by input row, NaN for a row that is not loaded; loaded [N]"""
    N = len(rows)
    nonnan = (~np.isnan(rows)).sum(1)
    first = np.where(np.isnan(rows).any(1), np.isnan(rows).argmax(1), rows.shape[1])
    loaded = (nonnan > 0) & (nonnan == first) & (nonnan % 2 == 0) & (site >= 0) & (site < S3)
    idx = np.flatnonzero(loaded)
    cols = {lb: np.full(N, np.nan) for lb in FLABELS + list(MR.COLUMNS) + ULABELS}
    if idx.size:
        kinds, par = feature_par()
        ft = FR.features_ref(rows[idx], kinds, par, site[idx])
        for q, lb in enumerate(FLABELS):
            cols[lb][idx] = ft[q]
        for s in range(S3):
            i = idx[site[idx] == s]
            if i.size:
                mo = MR.moho_rows(rows[i], MOHO[s, 0], MOHO[s, 1], MOHOVS[s])
                for q, lb in enumerate(MR.COLUMNS):
                    cols[lb][i] = mo[:, q]
        cols["vpvs"][idx] = vpvs[idx].astype(np.float64)
        cols["noise[0]"][idx], cols["noise[1]"][idx] = noise[idx, 0], noise[idx, 1]
        cols["nlayers"][idx] = MR.nlayers(rows[idx])
    return cols, loaded


def case(ML, dtype, N, device):
    """one input, built once: rows (family "a": depths on the grid of 0.25 km, vs on that of 0.25 km/s), interleaved sites, NaN rows
    among them; the device input also holds malformed rows and rows of site -1"""
    key = (ML, np.dtype(dtype).str, N, device)
    if key in _CASES:
        return _CASES[key]
    rs = np.random.RandomState(500 + 11 * ML + N)
    rows = make_rows(rs, N, ML, dtype, "a")
    site = rs.choice(np.arange(S3, dtype=np.int32), N) if N > 1 else np.array([1], np.int32)
    if N >= 63:
        rows[[5, N - 2]] = np.nan                                     # NaN rows: not loaded
    if device and N >= 63:
        bad = rows[:2].copy()
        bad[0, :] = np.nan
        bad[0, :3] = (3.0, 3.5, 10.0)                                 # an odd number of values
        bad[1, 2 * ML - 1] = 1.0 if np.isnan(bad[1, 2 * ML - 1]) else np.nan
        bad[1, 0] = np.nan                                            # the values are no prefix
        extra = np.concatenate((bad, rows[7:9]))                      # two malformed rows, two rows of site -1
        es = np.array([0, 2, -1, -1], np.int32)
        at = N // 2
        rows = np.concatenate((rows[:at], extra, rows[at:]))
        site = np.concatenate((site[:at], es, site[at:]))
    n = len(rows)
    vpvs = rs.choice(np.array([1.5, 1.75, 2.0, np.nan]), n).astype(dtype)
    noise = np.stack((rs.uniform(0, 1, n), rs.choice(np.array([0.0, -0.0, 0.5, -0.5]), n)), axis=1)
    cols, loaded = columns_ref(rows, site, vpvs, noise)
    _CASES[key] = dict(rows=rows, site=site, vpvs=vpvs, noise=noise, cols=cols, loaded=loaded)
    return _CASES[key]


def middle(v, site, default):
    """[S3]: per site a value the column takes there -- the upper median of the site's values -- or the default"""
    out = np.full(S3, default, np.float64)
    for s in range(S3):
        x = np.sort(v[(site == s) & ~np.isnan(v)])
        if x.size:
            out[s] = x[x.size // 2]
    return out


def rules(c):
    """the rules of one case: name -> (classes dict, K)"""
    cols, site = c["cols"], c["site"]
    mm, cm, nm = middle(cols["moho"], site, 30.0), middle(cols["crust"], site, 3.0), middle(cols["nlayers"], site, 2.0)
    main = {"shallow_lvz": [("moho", MOHO[:, 0], mm), ("lvz.depth", "has")],       # per-site bounds; a value exactly on hi: out
            "shallow": [("moho", -INF, mm)],
            "deep_thick": [("moho", mm, INF), ("nlayers", nm, INF), ("noise[1]", -0.0, INF)],   # exactly on lo: in; -0.0 <= 0.0
            "nomoho": [("moho", "lacks"), ("vpvs", "has"), ("crust", cm, INF)],
            "rest": []}
    edges = np.linspace(1.5, 5.0, 17)
    k16 = {"c%02d" % k: [("crust", edges[k], edges[k + 1]), ("n40", 0.0, INF), ("nlayers", "has"), ("vsjump", -INF, [INF, 1.0, 0.75])]
           for k in range(16)}
    return dict(main=main, one_all={"all": []}, one_term={"lvz": [("lvz.jump", -INF, -0.75)]}, k16=k16,
                gap={"a": [("vpvs", "lacks")], "b": [], "never": [("moho", "has")]})


def classify(c, classes, memspace, engine, **kw):
    import bayhunter_amd as bh
    m, st, vp, no = c["rows"], c["site"], c["vpvs"], c["noise"]
    if memspace == "device":
        import torch
        m, st, vp, no = (torch.from_numpy(v).cuda() for v in (m, st, vp, no))
    return bh.posterior_classes(m, classes, site=st, features=FEATS, moho=MOHO, mohovs=MOHOVS, columns=dict(vpvs=vp, noise=no),
                                nlayers=True, engine=engine, nsites=S3, **kw)


def host(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


@pytest.mark.parametrize("memspace", ["host", "device"])
@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("ML, dtype", [(6, np.float32), (6, np.float64), (32, np.float32), (32, np.float64)],
                         ids=lambda v: getattr(v, "__name__", str(v)))
def test_classes_and_counts_are_the_restatements(ML, dtype, N, memspace, engine):
    c = case(ML, dtype, N, memspace == "device")
    site, loaded, n = c["site"], c["loaded"], len(c["rows"])
    extra = 4 if memspace == "device" and N >= 63 else 0
    assert n == N + extra and loaded.sum() == N - (2 if N >= 63 else 0)
    for name, classes in rules(c).items():
        names, terms = CR.rule_terms(classes)
        K = len(names)
        want, wcounts = CR.classify(c["cols"], terms, K, site, loaded, S3)
        got = classify(c, classes, memspace, engine)
        cls = host(got["cls"])
        if memspace == "device":
            assert hasattr(got["cls"], "is_cuda") and got["cls"].is_cuda and got["site"].is_cuda
        else:
            assert isinstance(got["cls"], np.ndarray)
        assert cls.dtype == np.int32 and cls.shape == (n,)
        bad = np.flatnonzero(cls != want)
        assert not bad.size, (name, bad[:10], cls[bad[:10]], want[bad[:10]])
        assert got["names"] == names and got["nclasses"] == K and got["nsites"] == S3 * K
        assert np.array_equal(got["counts"], wcounts[:, :K]) and np.array_equal(got["unclassified"], wcounts[:, K]), name
        rows = np.array([np.sum(loaded & (site == s)) for s in range(S3)])
        assert np.array_equal(got["rows"], rows) and np.array_equal(got["counts"].sum(1) + got["unclassified"], rows)
        assert (cls[~loaded] == -1).all()
        with np.errstate(invalid="ignore"):
            assert np.array_equal(got["probability"], np.where(rows[:, None] > 0, wcounts[:, :K] / rows[:, None], np.nan), equal_nan=True)
        vs = host(got["site"])
        assert vs.dtype == np.int32 and np.array_equal(vs, np.where((want >= 0) & (site >= 0), site * K + want, -1))
        if name == "one_all":
            assert np.array_equal(cls, np.where(loaded, 0, -1))
        if N == 1000:     # no vacuous pass: every class of the main rule holds rows, as do the edges of its bounds
            if name == "main":
                assert (wcounts[:, :K].sum(0) > 0).all() and wcounts[:, K].sum() == 0, wcounts
                cols = c["cols"]
                mm = middle(cols["moho"], site, 30.0)[np.clip(site, 0, S3 - 1)]
                assert (loaded & (cols["moho"] == mm)).sum() >= S3
                assert (loaded & (cols["noise[1]"] == 0.0) & np.signbit(cols["noise[1]"])).any()
                assert (loaded & (cols["noise[1]"] == 0.0) & ~np.signbit(cols["noise[1]"]) & (want == 2)).any()
            if name == "k16":
                assert (wcounts[:, :16].sum(0) > 0).sum() >= 8 and wcounts[:, 16].sum() > 0, wcounts
            if name == "gap":
                assert wcounts[:, 0].sum() > 0 and wcounts[:, 1].sum() > 0 and wcounts[:, 2].sum() == 0 and wcounts[:, 3].sum() == 0


def test_a_site_alone_among_others_permuted_and_again(engine):
    import bayhunter_amd as bh
    c = case(32, np.float64, 257, False)
    classes = rules(c)["main"]
    a = classify(c, classes, "host", engine)
    b = classify(c, classes, "host", engine)
    assert np.array_equal(a["cls"], b["cls"]) and np.array_equal(a["counts"], b["counts"])                       # again
    d = classify(c, classes, "device", engine)
    assert np.array_equal(a["cls"], host(d["cls"])) and np.array_equal(a["counts"], d["counts"])                # from device memory
    perm = np.random.RandomState(3).permutation(257)
    p = classify({k: c[k][perm] for k in ("rows", "site", "vpvs", "noise")}, classes, "host", engine)
    assert np.array_equal(p["cls"], a["cls"][perm]) and np.array_equal(p["counts"], a["counts"])                 # the rows permuted
    for s in range(S3):                                                                                          # a site alone
        i = c["site"] == s
        own = {name: [tuple(np.asarray(v)[s] if np.ndim(v) else v for v in t) for t in ts] for name, ts in classes.items()}
        feats = {k: tuple(np.asarray(v)[s] if np.ndim(v) else v for v in f) for k, f in FEATS.items()}
        r = bh.posterior_classes(c["rows"][i], own, features=feats, moho=MOHO[s], mohovs=MOHOVS[s],
                                 columns=dict(vpvs=c["vpvs"][i], noise=c["noise"][i]), nlayers=True, engine=engine)
        assert np.array_equal(r["cls"], a["cls"][i]) and np.array_equal(r["counts"][0], a["counts"][s])
        assert r["unclassified"][0] == a["unclassified"][s] and np.array_equal(r["site"], r["cls"])


@pytest.mark.parametrize("memspace", ["host", "device"])
def test_the_exported_columns_are_the_restatements(memspace, engine):
    from bayhunter_amd import engine as E
    from bayhunter_amd.posterior import _Loaded
    c = case(32, np.float32, 257, memspace == "device")
    got = classify(c, {"all": []}, memspace, engine, return_columns=True)
    assert sorted(got["columns"]) == sorted(c["cols"])
    for lb, want in c["cols"].items():
        v = host(got["columns"][lb])
        assert v.dtype == np.float64 and v.shape == want.shape
        assert np.array_equal(v, want, equal_nan=True), lb
        assert np.isnan(v[~c["loaded"]]).all()
    # through the C ABI with a row stride above the set's columns: what lies beyond them is not touched
    m, st = c["rows"], c["site"]
    if memspace == "device":
        import torch
        m, st = torch.from_numpy(m).cuda(), torch.from_numpy(st).cuda()
    ld = _Loaded(m, st, engine, S3, scalars=True)
    try:
        ld.moho(MOHO[:, 0], MOHO[:, 1], MOHOVS)
        n = len(c["rows"])
        if memspace == "device":
            out = torch.full((n, 6), -7.0, dtype=torch.float64, device="cuda")
            ptr, mem, stream = C.c_void_p(out.data_ptr()), E.DEVICE, C.c_void_p(torch.cuda.current_stream().cuda_stream)
        else:
            out = np.full((n, 6), -7.0)
            ptr, mem, stream = C.c_void_p(out.ctypes.data), E.HOST, None
        engine._check(engine._L.bh_posterior_scalar_export(ld._p, E.SCALARS_MOHO, mem, stream, 6, ptr))
        out = host(out)
        assert (out[:, 4:] == -7.0).all()
        for q, lb in enumerate(MR.COLUMNS):
            assert np.array_equal(out[:, q], c["cols"][lb], equal_nan=True), lb
        rc = engine._L.bh_posterior_scalar_export(ld._p, E.SCALARS_MOHO, mem, stream, 3, ptr)
        assert rc == E.BH_EINVAL
        with pytest.raises(E.EngineError, match="ld must be at least"):
            engine._check(rc)
        rc = engine._L.bh_posterior_scalar_export(ld._p, E.SCALARS_FEATURES, mem, stream, 6, ptr)
        assert rc == E.BH_EINVAL
        with pytest.raises(E.EngineError, match="does not exist yet"):
            engine._check(rc)
    finally:
        ld.close()


# ---- conditioning is subsetting -------------------------------------------------------------------------------------------------

SPLIT_N = 1200     # about 400 rows per site


def split_case():
    """1200 float32 rows of 6 layers over three sites and a rule of four classes -- the Moho above or below the site's middle Moho,
    with or without a velocity drop -- that leaves the rows without a Moho in no class"""
    if "split" not in _CASES:
        rs = np.random.RandomState(77)
        rows = make_rows(rs, SPLIT_N, 6, np.float32, "a")
        site = rs.choice(np.arange(S3, dtype=np.int32), SPLIT_N)
        vpvs = rs.choice(np.array([1.5, 1.75, 2.0, np.nan]), SPLIT_N).astype(np.float32)
        noise = np.stack((rs.uniform(0, 1, SPLIT_N), rs.choice(np.array([0.0, 0.5, -0.5]), SPLIT_N)), axis=1)
        cols, loaded = columns_ref(rows, site, vpvs, noise)
        assert loaded.all()
        mm = middle(cols["moho"], site, 30.0)
        classes = {"shallow_lvz": [("moho", -INF, mm), ("lvz.depth", "has")], "shallow": [("moho", -INF, mm)],
                   "deep_lvz": [("moho", mm, INF), ("lvz.depth", "has")], "deep": [("moho", "has")]}
        names, terms = CR.rule_terms(classes)
        cls, counts = CR.classify(cols, terms, 4, site, loaded, S3)
        assert (counts >= 10).all(), counts                         # every class of every site holds rows, and so does "no class"
        misfits = rs.uniform(0.5, 3.0, SPLIT_N)
        c = dict(rows=rows, site=site, vpvs=vpvs, noise=noise, cols=cols, loaded=loaded, classes=classes, names=names, cls=cls,
                 counts=counts, misfits=misfits)
        _CASES["split"] = c
    return _CASES["split"]


def six_calls(bh, m, site, s, vpvs, noise, misfits, engine, **kw):
    """the six functions on rows m; s: the site whose per-site numbers they take (None: all three sites')"""
    pick = (lambda v: v) if s is None else (lambda v: np.asarray(v)[s])
    feats = {k: tuple(pick(v) if np.ndim(v) else v for v in f) for k, f in FEATS.items()}
    cols = dict(vpvs=vpvs, noise=noise)
    return dict(
        models=bh.posterior_models(m, site=site, dep_int=np.linspace(0, 60, 25), misfits=misfits, quantiles=(0.025, 0.975), engine=engine, **kw),
        hist2d=bh.posterior_hist2d(m, site=site, engine=engine, **kw),
        moho=bh.posterior_moho(m, site=site, moho=pick(MOHO), mohovs=pick(MOHOVS), bins=20, quantiles=(0.16, 0.84), engine=engine, **kw),
        scalars=bh.posterior_scalars(m, cols, site=site, engine=engine, **kw),
        features=bh.posterior_features(m, feats, site=site, bins=20, engine=engine, **kw),
        covariance=bh.posterior_covariance(m, site=site, dep_int=[10.0, 30.0], moho=pick(MOHO), mohovs=pick(MOHOVS), engine=engine, **kw))


def alone_results(engine):
    """{(site, class name): the six functions on the rows of that class alone} -- computed once, from host rows"""
    import bayhunter_amd as bh
    c = split_case()
    if "alone" not in c:
        out = {}
        for s in range(S3):
            for k, name in enumerate(c["names"]):
                i = (c["site"] == s) & (c["cls"] == k)
                out[s, name] = six_calls(bh, c["rows"][i], None, s, c["vpvs"][i], c["noise"][i], c["misfits"][i], engine)
        c["alone"] = out
    return c["alone"]


@pytest.mark.parametrize("memspace", ["host", "device"])
def test_conditioning_is_subsetting(memspace, engine):
    import bayhunter_amd as bh
    c = split_case()
    alone = alone_results(engine)
    cl = classify(c, c["classes"], memspace, engine)
    assert np.array_equal(host(cl["cls"]), c["cls"]) and np.array_equal(cl["counts"], c["counts"][:, :4])
    m, st, vp, no, mis = c["rows"], c["site"], c["vpvs"], c["noise"], c["misfits"]
    if memspace == "device":
        import torch
        m, st, vp, no = (torch.from_numpy(v).cuda() for v in (m, st, vp, no))
    res = six_calls(bh, m, st, None, vp, no, mis, engine, nsites=S3, classes=cl)
    unclassified = int(c["counts"][:, 4].sum())
    assert unclassified > 0
    for fn, r in res.items():
        assert isinstance(r, list) and len(r) == S3
        for s in range(S3):
            assert list(r[s]) == c["names"]
            for k, name in enumerate(c["names"]):
                got, want = dict(r[s][name]), dict(alone[s, name][fn])
                n = int(c["counts"][s, k])
                if fn in ("models", "hist2d"):
                    assert got["count"] == n and got["invalid_rows"] == 0
                elif fn == "covariance":
                    assert got["n"] + got["masked"] == n
                else:   # rows in no class: removed before a host load, site -1 and counted in `dropped` on the device
                    assert got["rows"] == n and got["invalid_rows"] == 0
                    assert got.pop("dropped") == (unclassified if memspace == "device" else 0) and want.pop("dropped") == 0
                same(got, want, (fn, s, name))
    # without classes= every result is what it was, and a dict of other rows is refused
    with pytest.raises(ValueError, match="same rows"):
        bh.posterior_hist2d(m[:100], site=st[:100], nsites=S3, classes=cl, engine=engine)
    with pytest.raises(ValueError, match="same site"):
        bh.posterior_hist2d(m, classes=cl, engine=engine)


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def test_refusals_leave_cls_and_counts_untouched(engine):
    from bayhunter_amd import engine as E
    from bayhunter_amd.posterior import _Loaded
    L = engine._L
    c = case(6, np.float64, 257, False)
    n = len(c["rows"])
    ld = _Loaded(c["rows"], c["site"], engine, S3, scalars=True)
    bare = _Loaded(c["rows"], c["site"], engine, S3, scalars=False)
    cls, counts = np.full(n, -7, np.int32), np.full((S3, 18), -7, np.int64)

    def call(h, K, tc, ts, tq, to, lo, hi, T=None):
        tc, ts, tq, to = (np.ascontiguousarray(v, np.int32) for v in (tc, ts, tq, to))
        T = tc.size if T is None else T
        lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, np.float64), (S3, max(T, 1))))
        hi = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, np.float64), (S3, max(T, 1))))
        pad = [np.ascontiguousarray(np.resize(v, max(T, 1))) for v in (tc, ts, tq, to)]
        return L.bh_posterior_classes(h._p, K, T, *[_ptr(v) for v in pad], _ptr(lo), _ptr(hi), E.HOST, None, _ptr(cls), _ptr(counts))

    def refused(rc, text):
        assert rc == E.BH_EINVAL
        with pytest.raises(E.EngineError, match=text):
            engine._check(rc)
        assert (cls == -7).all() and (counts == -7).all()

    try:
        M, U, F = E.SCALARS_MOHO, E.SCALARS_USER, E.SCALARS_FEATURES
        refused(call(ld, 1, [0], [M], [0], [E.CLASS_HAS], 0, 1), "term 0: the set does not exist yet")        # no set formed yet
        ld.moho(MOHO[:, 0], MOHO[:, 1], MOHOVS)
        refused(call(ld, 1, [0], [F], [0], [E.CLASS_HAS], 0, 1), "term 0: the set does not exist yet")        # MOHO formed, FEATURES not
        refused(call(ld, 2, [0, 1], [M, U], [0, 0], [E.CLASS_IN, E.CLASS_LACKS], 0, 1), "term 1: the set does not exist yet")
        refused(call(ld, 1, [0], [3], [0], [E.CLASS_HAS], 0, 1), "term 0: the set must be")                   # BH_SCALARS_DATA: no set of a rule
        refused(call(ld, 1, [0], [2], [0], [E.CLASS_HAS], 0, 1), "term 0: the set must be")
        lo = np.zeros((S3, 1))
        lo[2, 0] = np.nan
        refused(call(ld, 1, [0], [M], [0], [E.CLASS_IN], lo, 1), "term 0: site 2: a bound is NaN")
        refused(call(ld, 1, [0], [M], [0], [E.CLASS_IN], 0, np.nan), "term 0: site 0: a bound is NaN")
        lo = np.zeros((S3, 1))
        lo[1, 0] = 1.5
        refused(call(ld, 1, [0], [M], [0], [E.CLASS_IN], lo, 1), "term 0: site 1: lo > hi")
        refused(call(ld, 0, [], [], [], [], 0, 1), "K: 1..BH_CLASSES_MAX")
        refused(call(ld, 17, [], [], [], [], 0, 1), "K: 1..BH_CLASSES_MAX")
        refused(call(ld, 1, [0] * 65, [M] * 65, [0] * 65, [E.CLASS_HAS] * 65, 0, 1), "T: 0..BH_CLASS_MAXTERMS")
        refused(call(ld, 1, [0], [M], [0], [E.CLASS_HAS], 0, 1, T=-1), "T: 0..BH_CLASS_MAXTERMS")
        refused(call(ld, 1, [0], [M], [4], [E.CLASS_HAS], 0, 1), "term 0: column outside the set")
        refused(call(ld, 1, [0], [M], [-1], [E.CLASS_HAS], 0, 1), "term 0: column outside the set")
        refused(call(ld, 2, [1, 0], [M, M], [0, 0], [E.CLASS_HAS] * 2, 0, 1), "term 1: term_class must ascend")
        refused(call(ld, 2, [0, 2], [M, M], [0, 0], [E.CLASS_HAS] * 2, 0, 1), r"term 1: term_class outside \[0, K\)")
        refused(call(ld, 1, [0], [M], [0], [3], 0, 1), "term 0: no such op")
        refused(call(bare, 1, [], [], [], [], 0, 1), "bh_posterior_keep_rows")
        # NaN bounds and lo > hi of a term that reads none are no error; the handle still works
        assert call(ld, 1, [0], [M], [0], [E.CLASS_HAS], np.nan, np.nan) == E.BH_OK
        want, wcounts = CR.classify(c["cols"], [(0, "moho", "has", 0, 0)], 1, c["site"], c["loaded"], S3)
        assert np.array_equal(cls, want) and np.array_equal(counts.reshape(-1)[:S3 * 2].reshape(S3, 2), wcounts)
        assert (counts.reshape(-1)[S3 * 2:] == -7).all()
    finally:
        ld.close()
        bare.close()


def test_posterior_classes_refuses_what_check_classes_refuses(engine):
    import bayhunter_amd as bh
    c = case(6, np.float64, 257, False)
    with pytest.raises(ValueError, match="class 'a': 'moho' is no column of this call"):
        bh.posterior_classes(c["rows"], {"a": [("moho", 1, 2)]}, site=c["site"], features=FEATS, engine=engine)
    with pytest.raises(ValueError, match="class 'a', column 'moho', site 1: lo = 40.0 lies above hi = 35.0"):
        bh.posterior_classes(c["rows"], {"a": [("moho", [30, 40, 30], 35)]}, site=c["site"], moho=MOHO, engine=engine)
    with pytest.raises(ValueError, match="names two columns"):
        bh.posterior_classes(c["rows"], {"a": []}, site=c["site"], moho=MOHO, columns=dict(moho=np.zeros(len(c["rows"]))), engine=engine)


# ---- a recorded run end to end ---------------------------------------------------------------------------------------------------

def test_classes_of_a_recorded_run(site_run):  # noqa: F811
    import bayhunter_amd as bh
    dev = site_run
    pm = dev.posterior_moho()
    z = [tuple(float(v) for v in dev.site_priors[s]["z"]) for s in range(2)]
    # the split: the site's posterior median of the Moho depth; a site whose short run has no Moho row (the narrow priors of site
    # 1 keep vs below mohovs) takes the middle of its range, and all of its rows go to "none"
    med = np.array([pm[s]["moho"]["median"] if pm[s]["count"] else (z[s][0] + z[s][1]) / 2 for s in range(2)])
    assert not np.isnan(med).any() and any(pm[s]["count"] for s in range(2))
    classes = {"shallow": [("moho", -INF, med)], "deep": [("moho", med, INF)], "none": [("moho", "lacks")]}
    cl = dev.posterior_classes(classes, moho=True)
    assert cl["names"] == ["shallow", "deep", "none"] and cl["nsites"] == 6 and cl["cls"].is_cuda
    assert cl["selection"] == ("p2", False, ())
    assert (cl["unclassified"] == 0).all()
    got = dev.posterior_models(classes=cl)
    for s in range(2):
        h = dev.samples("p2", site=s)
        n = h["models"].shape[0] * h["models"].shape[1]
        m = h["models"].reshape(n, -1)
        mo = MR.moho_rows(m, z[s][0], z[s][1], 4.2)
        assert len(mo) == n
        own = {name: [tuple(np.asarray(v)[s] if np.ndim(v) else v for v in t) for t in ts] for name, ts in classes.items()}
        names, terms = CR.rule_terms(own)
        want, wcounts = CR.classify(dict(moho=mo[:, 0]), terms, 3, None, np.ones(n, bool), 1)
        assert np.array_equal(cl["counts"][s], wcounts[0, :3]) and cl["rows"][s] == n
        assert wcounts[0, 2] == n - pm[s]["count"]
        if pm[s]["count"] > 1:
            assert wcounts[0, 0] > 0 and wcounts[0, 1] > 0                                # the median splits the rows with a Moho
        hc = bh.posterior_classes(m, own, moho=z[s], engine=dev.engine)
        assert np.array_equal(hc["cls"], want)
        same(got[s], bh.posterior_models(m, misfits=h["misfits"][..., -1].reshape(n), classes=hc, engine=dev.engine), (s, "models"))
    with pytest.raises(ValueError, match="phase"):
        dev.posterior_models(classes=cl, phase="p1")
    with pytest.raises(ValueError, match="exclude_chains"):
        dev.posterior_moho(classes=cl, exclude_chains=(1,))
