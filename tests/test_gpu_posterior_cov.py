"""Posterior covariance and correlation on the GPU (include/bh_engine_posterior_cov.h; bayhunter_amd.posterior_covariance,
DeviceChains.posterior_covariance, covariance_from_storage) against the restatement in integers and rationals (tests/cov_ref.py):
n, masked, L, x0, exact, s and raw as integers, mean, cov and corr within 1 ulp of the rationals."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
import cov_ref as CR
import moho_ref as MR
from test_gpu_posterior_quantiles import same, synth
from test_gpu_posterior_scalars import crust_rows

pytestmark = pytest.mark.gpu
KEYS = ("f32", "f64of32", "f64")
M28 = (1 << 28) - 1
RAW = ("n", "masked", "L", "x0", "exact", "s", "raw")
ALL = RAW + ("mean", "cov", "corr")


@pytest.fixture(scope="module")
def G():
    return golden("posterior_golden.npz")


def ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def loaded(models, site=None, engine=None, nsites=None, scalars=True):
    from bayhunter_amd.posterior import _Loaded
    return _Loaded(models, site, engine, nsites, scalars=scalars)


def prefilled(S, P):
    npair = P * (P + 1) // 2
    u64 = lambda *sh: np.full(sh, 0xA5A5A5A5A5A5A5A5, np.uint64)
    return dict(n=u64(S).view(np.int64), masked=u64(S).view(np.int64), L=np.full((S, P), 0xA5A5A5A5, np.uint32).view(np.int32),
                x0=u64(S, P).view(np.int64), exact=np.full((S, P), 0xA5A5A5A5, np.uint32).view(np.int32), s=u64(S, P),
                raw=u64(S, npair, 3), mean=u64(S, P).view(np.float64), cov=u64(S, P, P).view(np.float64),
                corr=u64(S, P, P).view(np.float64))


def call(ld, dep, which=-1, cols=(), D=None, Qc=None, S=None):
    """bh_posterior_cov with prefilled outputs: (rc, outputs)"""
    dep = np.ascontiguousarray(dep, np.float64)
    cols = np.ascontiguousarray(cols, np.int32)
    o = prefilled(ld.S if S is None else S, max(dep.size + cols.size, 1))
    rc = ld._L.bh_posterior_cov(ld._p, dep.size if D is None else D, ptr(dep), int(which), cols.size if Qc is None else Qc, ptr(cols),
                                *[ptr(o[k]) for k in ALL])
    return rc, o


def bits(o):
    return {k: np.ascontiguousarray(v).view(np.uint8).copy() for k, v in o.items()}


def same_bits(a, b, keys=ALL, sites=None):
    """the outputs a and b (of the sites `sites` = (site of a, site of b) or all) are the same bits"""
    for k in keys:
        x, y = (a[k], b[k]) if sites is None else (a[k][sites[0]], b[k][sites[1]])
        assert x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), k


def check_site(o, s, V, masked=0, I=None):
    """site s of the outputs against the restatement of its table V"""
    I = CR.integers(V) if I is None else I
    P = V.shape[1]
    assert int(o["n"][s]) == I["n"] and int(o["masked"][s]) == masked
    assert [int(v) for v in o["L"][s]] == I["L"] and [int(v) for v in o["x0"][s]] == I["x0"], (o["L"][s], I["L"])
    assert [int(v) for v in o["exact"][s]] == I["exact"]
    assert [int(v) for v in o["s"][s]] == I["s"]
    got = [[int(v) for v in r] for r in o["raw"][s]]
    if got != I["raw"]:
        k = [i for i, (a, b) in enumerate(zip(got, I["raw"])) if a != b]
        raise AssertionError("raw differs at %d of %d pairs, first %r: %r, want %r" % (len(k), len(got), CR.pairs(P)[k[0]], got[k[0]], I["raw"][k[0]]))
    bad = CR.check_finished(o["mean"][s], o["cov"][s], o["corr"][s], I["n"], I["L"], I["x0"], I["s"], I["raw"])
    assert not bad, bad[:5]
    return I


def grid(D):
    return np.array([20.0]) if D == 1 else np.linspace(0, 70, D)


# ---- the golden rows ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", KEYS)
def test_golden_rows_give_the_restated_integers_and_numbers_within_an_ulp(G, key, engine):
    m, dep = G[key + "_models"], G["dep_int"]
    ld = loaded(m, engine=engine, scalars=False)
    try:
        rc, o = call(ld, dep)
        assert rc == 0
    finally:
        ld.close()
    I = check_site(o, 0, G[key + "_vsi"])
    if key == "f64":
        assert not np.all(o["exact"] == 1)        # 2^52.5 lowest bits wide: rounded -- and the sums are those of the rounded values
    else:
        assert np.all(o["exact"] == 1)
    assert I["n"] == len(G[key + "_vsi"]) == 1781


# ---- shapes at the edges of the tiling --------------------------------------------------------------------------------------

DS = (1, 15, 16, 17, 33, 64, 65, 130)   # one tile; a tile's edge from both sides; two and three tile columns; one, two, three groups of 64
NROWS = (1, 2, 3, 5, 8191, 8192, 8193, 8192 + 5)


@pytest.mark.parametrize("N", NROWS)
def test_depth_counts_and_row_counts_at_the_edges(N, engine):
    """every D over every number of rows (rows that are no multiple of the 4 of an MFMA or of the 16 of a step; both sides of a chunk
    of 8192), float32 and float64 rows by turns; then D = 14 + 2 scalar columns (P crosses a tile) and scalar columns alone"""
    kind = KEYS[NROWS.index(N) % 3]
    rs = np.random.RandomState(N)
    m = synth(rs, N, 6, kind)
    u = np.stack((rs.normal(0, 1, N), rs.uniform(1.6, 1.9, N).astype(np.float32)), axis=1)
    ld = loaded(m, engine=engine)
    try:
        ld.attach(u, False)
        big = DS if N in (5, 8193) else DS[:5]
        for D in big:
            rc, o = call(ld, grid(D))
            assert rc == 0
            check_site(o, 0, CR.table(m, grid(D))[0])
        rc, o = call(ld, grid(14), 1, (0, 1))
        assert rc == 0
        check_site(o, 0, CR.table(m, grid(14), u)[0])
        rc, o = call(ld, np.zeros(0), 1, (1, 0))
        assert rc == 0
        check_site(o, 0, u[:, ::-1].astype(np.float64))
    finally:
        ld.close()


# ---- the contract -----------------------------------------------------------------------------------------------------------

def test_sites_alone_among_others_permuted_from_device_and_again(engine):
    """three sites of unequal counts, an empty one between them: each equals the restatement, itself loaded alone, the rows
    permuted, the rows on the device and a second call -- on bits, every output"""
    import torch
    rs = np.random.RandomState(11)
    per = [synth(rs, 700, 6, "f32"), synth(rs, 0, 6, "f32").reshape(0, 12), synth(rs, 8200, 6, "f32")]
    per[0][5, 0] = np.float32(2.0)
    u = [np.stack((rs.normal(0, 1, len(p)), rs.uniform(0, 1, len(p))), axis=1).astype(np.float32) for p in per]
    u[0][3, 1] = np.nan                                                  # one row of site 0 is left out
    rows, site = np.concatenate(per), np.concatenate([np.full(len(p), s, np.int32) for s, p in enumerate(per)])
    uu = np.concatenate(u)
    dep = grid(17)

    def run(rows, site, uu, nsites):
        ld = loaded(rows, site, engine=engine, nsites=nsites)
        try:
            ld.attach(uu, False)
            rc, o = call(ld, dep, 1, (0, 1))
            rc2, o2 = call(ld, dep, 1, (0, 1))
            assert rc == 0 and rc2 == 0
            same_bits(o, o2)
            return o
        finally:
            ld.close()

    o = run(rows, site, uu, 3)
    for s in (0, 2):
        V, masked = CR.table(per[s], dep, u[s])
        check_site(o, s, V, masked)
    assert (o["n"][0], o["masked"][0], o["n"][1], o["masked"][1]) == (699, 1, 0, 0)
    assert np.isnan(o["mean"][1]).all() and np.isnan(o["cov"][1]).all() and np.isnan(o["corr"][1]).all()
    assert np.all(o["L"][1] == 0) and np.all(o["x0"][1] == 0) and np.all(o["exact"][1] == 1) and not o["s"][1].any() and not o["raw"][1].any()
    for s in (0, 2):                                                     # alone
        same_bits(o, run(per[s], None, u[s], None), sites=(s, 0))
    perm = rs.permutation(len(rows))
    same_bits(o, run(rows[perm], site[perm], uu[perm], 3))
    dev = run(torch.from_numpy(rows[perm]).cuda(), torch.from_numpy(site[perm]).cuda(), torch.from_numpy(uu[perm]).cuda(), 3)
    same_bits(o, dev)


# ---- the limbs ----------------------------------------------------------------------------------------------------------------

def test_the_largest_accumulators_of_a_chunk_are_exact(engine):
    """8192 rows, one chunk: a column at 2^28 - 1 in every row but the one that holds its minimum 0 (Y = v - min: some row is 0),
    a column of zeros, a column alternating 0 and 2^28 - 1 and its mirror image: both limbs at 2^14 - 1, the sums as large as a
    chunk can make them"""
    N = 8192
    rs = np.random.RandomState(2)
    m = synth(rs, N, 4, "f32")
    u = np.zeros((N, 4))
    u[:, 0] = M28
    u[17, 0] = 0
    u[::2, 2] = M28
    u[:, 3] = M28 - u[:, 2]
    ld = loaded(m, engine=engine)
    try:
        ld.attach(u, False)
        rc, o = call(ld, np.zeros(0), 1, (0, 1, 2, 3))
        assert rc == 0
        I = check_site(o, 0, u)
        assert I["L"] == [0, 0, 0, 0] and I["raw"][0] == [(N - 1) * ((1 << 14) - 1) ** 2, 2 * (N - 1) * ((1 << 14) - 1) ** 2, (N - 1) * ((1 << 14) - 1) ** 2]
        assert np.isnan(o["corr"][0, 1]).all() and np.all(o["cov"][0, 1] == 0) and -1.0 <= o["corr"][0, 2, 3] <= -1.0 + 2.0 ** -53
        rc, o = call(ld, grid(16), 1, (0, 1, 2, 3))                      # ... beside depth columns: the scalar columns in a second tile
        assert rc == 0
        check_site(o, 0, CR.table(m, grid(16), u)[0])
    finally:
        ld.close()


def test_a_column_wider_than_two_limbs_is_rounded_as_the_restatement_rounds(engine):
    N = 37
    rs = np.random.RandomState(4)
    m = synth(rs, N, 4, "f64")
    u = np.tile(np.array([3.0, 3.0 + 2.0 ** -40, 7.5]), 13)[:N, None] + np.zeros((N, 2))
    u[:, 1] = rs.uniform(3.0, 7.5, N)                                    # general float64 values: ties and halves are not special
    ld = loaded(m, engine=engine)
    try:
        ld.attach(u, False)
        rc, o = call(ld, grid(3), 1, (0, 1))
        assert rc == 0
        I = check_site(o, 0, CR.table(m, grid(3), u)[0])
        assert I["exact"][3:] == [0, 0] and I["L"][3] == -25 and I["x0"][3] == 3 << 25
    finally:
        ld.close()


def test_degenerate_columns(engine):
    """a constant column: cov row 0, corr row NaN; a column twice and a column beside its negation: corr within 1 ulp of +-1 and inside"""
    N = 501
    rs = np.random.RandomState(8)
    m = synth(rs, N, 5, "f32")
    m[:, 0] = np.float32(3.25)                                           # the top layer: constant at depth 0 where it is thick enough
    x = rs.normal(0, 1, N)
    u = np.stack((x, -x, np.full(N, 1.75)), axis=1)
    dep = np.array([0.0, 20.0])
    ld = loaded(m, engine=engine)
    try:
        ld.attach(u, False)
        rc, o = call(ld, dep, 1, (0, 0, 1, 2))
        assert rc == 0
        V = CR.table(m, dep, u[:, [0, 0, 1, 2]])[0]
        assert np.all(V[:, 0] == 3.25)
        check_site(o, 0, V)
        cov, corr = o["cov"][0], o["corr"][0]
        for k in (0, 5):
            assert np.all(cov[k] == 0) and np.all(cov[:, k] == 0) and np.isnan(corr[k]).all() and np.isnan(corr[:, k]).all()
        assert 1.0 - 2.0 ** -53 <= corr[2, 3] <= 1.0 and -1.0 <= corr[2, 4] <= -1.0 + 2.0 ** -53 and corr[3, 4] == corr[2, 4]
        assert np.all(np.diagonal(corr)[1:5] == 1.0)
    finally:
        ld.close()


# ---- listwise deletion ------------------------------------------------------------------------------------------------------------

def test_rows_without_a_moho_leave_the_whole_matrix(engine):
    rs = np.random.RandomState(21)
    per = [crust_rows(rs, 300), crust_rows(rs, 8300)]
    rows, site = np.concatenate(per), np.repeat(np.arange(2, dtype=np.int32), [300, 8300])
    lo, hi, mv = np.array([5.0, 10.0]), np.array([30.0, 35.0]), np.array([4.0, 4.1])
    dep = grid(15)
    ld = loaded(rows, site, engine=engine, nsites=2)
    try:
        found = ld.moho(lo, hi, mv)
        rc, o = call(ld, dep, 0, (0, 2))
        assert rc == 0
        for s in range(2):
            mr = MR.moho_rows(per[s], lo[s], hi[s], mv[s])
            V, masked = CR.table(per[s], dep, mr[:, [0, 2]])
            assert 0 < found[s] < len(per[s]) and o["n"][s] == found[s] == len(V) and o["masked"][s] == len(per[s]) - found[s] == masked
            check_site(o, s, V, masked)                                  # (V: the kept rows alone, the vs block included)
        rc2, o2 = call(ld, dep)                                          # without the Moho columns every row is used
        assert rc2 == 0 and list(o2["n"]) == [300, 8300] and not np.array_equal(o2["mean"], o["mean"][:, :15])
    finally:
        ld.close()


def test_nan_in_a_user_column_masks_the_row_and_inf_is_refused(engine):
    from bayhunter_amd import engine as E
    rs = np.random.RandomState(22)
    N = 90
    m = synth(rs, N, 5, "f64of32")
    u = rs.normal(0, 1, (N, 3))
    u[4, 0] = u[9, 2] = u[30, 1] = u[30, 2] = np.nan
    dep = grid(5)
    ld = loaded(m, engine=engine)
    try:
        ld.attach(u, False)
        rc, o = call(ld, dep, 1, (0, 1, 2))
        V, masked = CR.table(m, dep, u)
        assert rc == 0 and masked == 3
        check_site(o, 0, V, 3)
        rc, o = call(ld, dep, 1, (1,))                                   # only the NaN of the chosen columns count
        assert rc == 0
        check_site(o, 0, *CR.table(m, dep, u[:, [1]]))
        u[50, 1] = np.inf
        ld.attach(u, False)
        before = bits(prefilled(1, 8))
        rc, o = call(ld, dep, 1, (0, 1, 2))
        assert rc == -1 and all(np.array_equal(bits(o)[k], before[k]) for k in ALL)
        with pytest.raises(E.EngineError, match="not finite"):
            engine._check(rc)
        rc, o = call(ld, dep, 1, (0, 2))                                 # ... the column with the inf is not among these
        assert rc == 0
    finally:
        ld.close()


# ---- errors -------------------------------------------------------------------------------------------------------------------

def test_refusals_carry_their_message_and_write_nothing(engine):
    from bayhunter_amd import engine as E
    rs = np.random.RandomState(3)
    m = synth(rs, 50, 6, "f32")
    dep = grid(5)

    def refused(res, text, S=1, P=5):
        rc, o = res
        want = bits(prefilled(S, P))
        assert rc == E.BH_EINVAL and all(np.array_equal(bits(o)[k], want[k]) for k in ALL), text
        with pytest.raises(E.EngineError, match=text):
            engine._check(rc)

    ld = loaded(m, engine=engine)
    try:
        refused(call(ld, dep, 0, (0,)), "MOHO set does not exist", P=6)
        refused(call(ld, dep, 1, (0,)), "USER set does not exist", P=6)
        ld.attach(rs.normal(0, 1, (50, 2)), False)
        refused(call(ld, np.array([0.0, 10.0, 10.0, 20.0, 30.0])), "ascending")
        refused(call(ld, np.array([0.0, 10.0, np.nan, 20.0, 30.0])), "ascending")
        refused(call(ld, np.zeros(0)), "BH_COV_MAXCOLS", P=1)                              # P = 0
        refused(call(ld, np.linspace(0, 90, 256), 1, (0,)), "BH_COV_MAXCOLS", P=257)      # P = 257
        refused(call(ld, dep, 1, (0, 2)), "column out of range", P=7)
        refused(call(ld, dep, 1, (-1,)), "column out of range", P=6)
        refused(call(ld, dep, -1, (0,)), "BH_SCALARS_MOHO or BH_SCALARS_USER", P=6)
        refused(call(ld, dep, 3, (0,)), "BH_SCALARS_MOHO or BH_SCALARS_USER", P=6)
        refused(call(ld, dep, D=-1), "BH_COV_MAXCOLS")
        rc, o = call(ld, np.linspace(0, 90, 255), 1, (0,))                                 # P = 256 is served
        assert rc == 0 and o["n"][0] == 50
    finally:
        ld.close()
    ld = loaded(m, engine=engine, scalars=False)                                           # rows loaded without keep_rows
    try:
        refused(call(ld, dep, 1, (0,)), "bh_posterior_keep_rows", P=6)
        rc, o = call(ld, dep)
        assert rc == 0
        check_site(o, 0, CR.table(m, dep)[0])
    finally:
        ld.close()
    lib = E.load_library()                                                                 # a handle that has loaded nothing
    h = C.c_void_p()
    engine._check(lib.bh_posterior_create(engine._h, C.byref(h)))
    try:
        fresh = type("H", (), dict(_L=lib, _p=h, S=1))()
        refused(call(fresh, dep), "no rows loaded")
    finally:
        lib.bh_posterior_destroy(h)
    # the cap on nsites * P (P + 1) / 2 cells
    ld = loaded(m, np.zeros(50, np.int32), engine=engine, nsites=600, scalars=False)
    try:
        rc, o = call(ld, np.linspace(0, 90, 256), S=1)                                     # 600 * 32896 > 2^24 (refused: writes nothing)
        assert rc == E.BH_EINVAL
        with pytest.raises(E.EngineError, match="BH_COV_MAXCELLS"):
            engine._check(rc)
        assert all(np.array_equal(bits(o)[k], bits(prefilled(1, 256))[k]) for k in ALL)
    finally:
        ld.close()


def test_the_widest_call_is_served(engine):
    """P = 256 = 255 depths and a scalar column: four groups of 64 a side, every tile in use"""
    rs = np.random.RandomState(31)
    N = 300
    m = synth(rs, N, 8, "f32")
    u = rs.normal(0, 1, (N, 1)).astype(np.float32)
    dep = np.linspace(0, 70, 255)
    ld = loaded(m, engine=engine)
    try:
        ld.attach(u, False)
        rc, o = call(ld, dep, 1, (0,))
        assert rc == 0
        check_site(o, 0, CR.table(m, dep, u)[0])
    finally:
        ld.close()


# ---- the public layer ---------------------------------------------------------------------------------------------------------

def check_public(r, V, dep, names, masked=0):
    I = CR.integers(V)
    assert r["n"] == I["n"] and r["masked"] == masked and r["names"] == [float(d) for d in dep] + list(names)
    assert np.array_equal(r["dep"], dep) and list(r["exact"]) == [bool(e) for e in I["exact"]] and r["exact"].dtype == bool
    bad = CR.check_finished(r["mean"], r["cov"], r["corr"], I["n"], I["L"], I["x0"], I["s"], I["raw"])
    assert not bad, bad[:5]
    with np.errstate(invalid="ignore"):
        assert np.array_equal(r["std"], np.sqrt(np.diagonal(r["cov"])), equal_nan=True)
    assert sorted(r) == ["corr", "cov", "dep", "exact", "masked", "mean", "n", "names", "std"]


def test_posterior_covariance_of_a_two_site_table(engine):
    import bayhunter_amd as bh
    rs = np.random.RandomState(41)
    per = [crust_rows(rs, 400).astype(np.float64), crust_rows(rs, 250, dtype=np.float64)]   # float32-exact values; general ones
    rows, site = np.concatenate(per), np.repeat(np.arange(2, dtype=np.int32), [400, 250])
    perm = rs.permutation(650)
    like = rs.normal(0, 1, 650)
    noise = rs.uniform(0, 1, (650, 2)).astype(np.float32)
    noise[7, 1] = np.nan
    dep = np.linspace(0, 60, 13)
    r = bh.posterior_covariance(rows[perm], site[perm], dep_int=dep, engine=engine)
    rc = bh.posterior_covariance(rows[perm], site[perm], dep_int=dep, columns=dict(likes=like[perm], noise=noise[perm]), engine=engine)
    rm = bh.posterior_covariance(rows[perm], site[perm], dep_int=dep, moho=[(5.0, 30.0), (10.0, 35.0)], mohovs=[4.0, 4.1], engine=engine)
    r0 = bh.posterior_covariance(rows[perm], site[perm], dep_int=[], moho=(5.0, 40.0), moho_columns=("vsjump", "moho", "vslast"),
                                 engine=engine)
    for s in range(2):
        sel = site == s
        check_public(r[s], CR.table(per[s], dep)[0], dep, ())
        u = np.concatenate((like[sel, None], noise[sel].astype(np.float64)), axis=1)
        check_public(rc[s], CR.table(per[s], dep, u)[0], dep, ("likes", "noise[0]", "noise[1]"), masked=1 if s == 0 else 0)
        mr = MR.moho_rows(per[s], (5.0, 10.0)[s], (30.0, 35.0)[s], (4.0, 4.1)[s])
        V, masked = CR.table(per[s], dep, mr[:, [0, 2]])
        check_public(rm[s], V, dep, ("moho", "vscrust"), masked)
        mr = MR.moho_rows(per[s], 5.0, 40.0, 4.2)
        V, masked = CR.table(per[s], np.zeros(0), mr[:, [3, 0, 1]])
        check_public(r0[s], V, np.zeros(0), ("vsjump", "moho", "vslast"), masked)
    one = bh.posterior_covariance(per[0], dep_int=dep, engine=engine)                        # no site: one dict, the same bits
    same(one, r[0])
    with pytest.raises(ValueError, match="one set"):
        bh.posterior_covariance(rows, site, columns=dict(likes=like), moho=(5.0, 30.0), engine=engine)
    with pytest.raises(ValueError, match="moho_columns"):
        bh.posterior_covariance(rows, site, moho=(5.0, 30.0), moho_columns=("depth",), engine=engine)
    with pytest.raises(ValueError, match="BH_COV_MAXCOLS"):
        bh.posterior_covariance(rows, site, dep_int=np.linspace(0, 90, 257), engine=engine)


DEP = np.linspace(0, 80, 33)


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    """the short recorded run of tests/test_gpu_posterior_quantiles.py: 2 sites x 4 chains under their own priors, 100 kept
    iterations each"""
    from bayhunter_amd.device_chains import DeviceChains
    from test_gpu_posterior_scalars import site_targets
    from test_gpu_sites_priors import SITE_INIT, SITE_PRIORS
    T, Cn = 100, 4
    path = str(tmp_path_factory.mktemp("cov"))
    inits = [dict(SITE_INIT[s], iter_burnin=100, iter_main=T, maxmodels=T, savepath=path) for s in range(2)]
    dc = DeviceChains(site_targets(), Cn, inits, SITE_PRIORS[:2], seed=78, search="fast", record="device").run()
    assert dc.thinning == 1 and dc.nsamples("p2") == T
    return dc, T, Cn, path


def test_chains_form_the_covariance_of_their_device_record(recorded, engine):
    import bayhunter_amd as bh
    from test_gpu_sites_priors import SITE_PRIORS
    dc, T, Cn, path = recorded
    n = T * Cn
    mv = [3.6, 3.8]
    a = dc.posterior_covariance(dep_int=DEP)
    b = dc.posterior_covariance(dep_int=DEP, scalars=("likes", "vpvs"))
    c = dc.posterior_covariance(dep_int=DEP, moho=True, mohovs=mv)
    ex = dc.posterior_covariance(dep_int=DEP, scalars=("likes",), exclude_chains=(1, 6))
    for s in range(2):
        h = dc.samples("p2", site=s)
        m = h["models"].reshape(n, -1)
        assert a[s]["n"] == n
        same(a[s], bh.posterior_covariance(m, dep_int=DEP, engine=engine), (s, "depths"))
        check_public(a[s], CR.table(m, DEP)[0], DEP, ())
        same(b[s], bh.posterior_covariance(m, dep_int=DEP, columns=dict(likes=h["likes"].reshape(n), vpvs=h["vpvs"].reshape(n)),
                                           engine=engine), (s, "scalars"))
        same(c[s], bh.posterior_covariance(m, dep_int=DEP, moho=SITE_PRIORS[s]["z"], mohovs=mv[s], engine=engine), (s, "moho"))
        assert c[s]["n"] + c[s]["masked"] == n and c[s]["names"][-2:] == ["moho", "vscrust"]
        keep = np.ones(Cn, bool)
        keep[[1] if s == 0 else [2]] = False                               # chains 1 | 6
        mk = h["models"][:, keep].reshape(T * 3, -1)
        same(ex[s], bh.posterior_covariance(mk, dep_int=DEP, columns=dict(likes=h["likes"][:, keep].reshape(T * 3)), engine=engine),
             (s, "excluded"))
    with pytest.raises(ValueError, match="no column of the store"):
        dc.posterior_covariance(scalars=("depth",))
    # the saved folders (no chain is an outlier at dev = 10)
    paths = dc.save(path)
    for p in paths:
        bh.save_final_distribution(p, maxmodels=10 * n, dev=10.0)
    fs = bh.covariance_from_storage(paths, dep_int=DEP, engine=engine)
    fm = bh.covariance_from_storage(paths, dep_int=DEP, moho=True, mohovs=mv, engine=engine)
    for s in range(2):
        cm = np.load(paths[s] + "/c_models.npy")
        assert len(cm) == n
        same(fs[s], bh.posterior_covariance(cm, dep_int=DEP, engine=engine), (s, "stored"))
        same(fm[s], bh.posterior_covariance(cm, dep_int=DEP, moho=SITE_PRIORS[s]["z"], mohovs=mv[s], engine=engine), (s, "stored moho"))
        check_public(fs[s], CR.table(cm, DEP)[0], DEP, ())


def test_tempered_chains_take_their_cold_rows(engine):
    """one ladder of 4 temperatures per site: the beta = 1 rows are selected on the device"""
    import bayhunter_amd as bh
    from bayhunter_amd.device_chains import DeviceChains
    from test_gpu_chains import SETUPS
    from test_gpu_posterior_scalars import site_targets
    su = SETUPS["exp"]
    T = 80
    init = dict(su["init"], iter_burnin=160, iter_main=T, maxmodels=T)
    ladder = np.repeat(np.arange(2), 4)
    betas = np.tile(1.0 / np.geomspace(1.0, 20.0, 4), 2)
    dc = DeviceChains(site_targets(), 4, init, su["priors"], seed=6, betas=betas, ladder=ladder, swap_every=20, record="device").run()
    cold = dc.posterior_covariance(dep_int=DEP, scalars=("likes",))                          # cold_only by default
    every = dc.posterior_covariance(dep_int=DEP, cold_only=False)
    for s in range(2):
        h = dc.samples("p2", cold_only=True, site=s)
        m = h["models"].reshape(T, -1)
        assert cold[s]["n"] == T and every[s]["n"] == 4 * T
        same(cold[s], bh.posterior_covariance(m, dep_int=DEP, columns=dict(likes=h["likes"].reshape(T)), engine=engine), (s, "cold"))
