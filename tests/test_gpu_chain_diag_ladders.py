"""The chain diagnostics of tempered runs on the GPU (include/bh_engine_chain_diag_ladders.h, bayhunter_amd/diagnostics.py): the ladder
index against the restatement tests/ladder_ref.py, exactly; the gathered sums, model series and medians against the existing calls on
the table gathered on the host, bit for bit, with every element of a chain that is not selected at a row a NaN (or a malformed model
row), so that a read of unselected data cannot pass; the refusals; and DeviceChains.ladder_diagnostics of a tempered run end to end."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import diag_ref as R
import ladder_ref as LR
from conftest import REPO, golden
import bayhunter_amd as bh
from bayhunter_amd import diagnostics as D
from bayhunter_amd import engine as E
from bayhunter_amd import results
from bayhunter_amd.device_chains import DeviceChains

pytestmark = pytest.mark.gpu

TILE, MAXLAG = E.DIAG_TILE, E.DIAG_MAXLAG
KEYS = D.FIELDS + ("p",)
FILL = -7777.0
NCHAINS = 5


def test_python_constants_mirror_the_header():
    txt = open(os.path.join(REPO, "include", "bh_engine_chain_diag_ladders.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define\s+(BH_LADDER_[A-Z]+)\s+(\d+)\b", txt, flags=re.M)}
    assert defs == {"BH_LADDER_MAXRUNGS": E.LADDER_MAXRUNGS} and E.LADDER_MAXRUNGS == 64
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert sorted(set(re.findall(r"\b(bh_[a-z_]+)\s*\(", txt))) == sorted(E.CHAIN_LADDER_SYMBOLS)
    lib = C.CDLL(E.LIB_PATH)
    assert all(hasattr(lib, n) for n in E.CHAIN_LADDER_SYMBOLS) and lib.bh_abi_version() == 10
    assert not set(E.CHAIN_LADDER_SYMBOLS) & set(E.CHAIN_DIAG_SYMBOLS) and len(E.CHAIN_DIAG_SYMBOLS) == 3


# ---- the ladder index -------------------------------------------------------------------------------------------------------------
def same_index(got, want, T):
    import torch
    for k in ("sel", "rung"):
        g = got[k].cpu().numpy() if isinstance(got[k], torch.Tensor) else got[k]
        assert g.dtype == np.int32 and np.array_equal(g, want[k]), k
    for k in ("occupancy", "round_trips", "moves", "ids"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), k
    assert len(got["members"]) == len(want["members"]) and all(np.array_equal(a, b) for a, b in zip(got["members"], want["members"]))
    assert np.all(got["occupancy"].sum(axis=1) == T)


LADDERS = {"interleaved": [0, 1, 0, 1, 2, 0, 1, 2, 2, 0],
           "sizes 1, 2, 5, 64": [7] + [3] * 2 + [11] * 5 + [0] * 64,
           "one ladder": [4] * 6}


@pytest.mark.parametrize("tie", [False, True])
@pytest.mark.parametrize("T", [1, 2, 7, 257])
@pytest.mark.parametrize("which", sorted(LADDERS))
def test_ladder_index_equals_the_restatement(engine, which, T, tie):
    """host and device memspace and a strided device view of beta (another ld_t, an offset; the gaps are NaN and must not be read)"""
    import torch
    ladder = LADDERS[which]
    beta = LR.permuted_betas(np.random.RandomState(T + len(ladder)), T, ladder, tie=tie)
    want = LR.ladder_index(beta, ladder)
    if T == 257:
        assert want["moves"].sum() > 0 and want["round_trips"].sum() > 0
    same_index(D.ladder_index(beta, ladder, engine=engine), want, T)
    dev = torch.device("cuda", 0)
    got = D.ladder_index(torch.from_numpy(beta).to(dev), ladder, engine=engine)
    assert got["sel"].is_cuda and got["rung"].is_cuda
    same_index(got, want, T)
    big = np.full((2 * T + 1, len(ladder) + 3), np.nan)
    big[1:2 * T + 1:2, 2:len(ladder) + 2] = beta
    tbig = torch.from_numpy(big).to(dev)
    view = tbig[1:2 * T + 1:2, 2:len(ladder) + 2]
    assert view.data_ptr() != tbig.data_ptr() and (T == 1 or view.stride(0) == 2 * big.shape[1])
    same_index(D.ladder_index(view, ladder, engine=engine), want, T)
    hview = big[1:2 * T + 1:2, 2:len(ladder) + 2]
    same_index(D.ladder_index(hview, ladder, engine=engine), want, T)
    # the cold mask rebuilt from sel is the rule of DeviceChains._cold_mask
    mask = np.zeros(beta.shape, bool)
    mask[np.arange(T)[:, None], got["sel"].cpu().numpy()] = True
    assert np.array_equal(mask, LR.cold_mask(beta, ladder))


def raw_index(engine, beta, ladder, K, R):
    """bh_chain_ladder_index on a contiguous host table with prefilled outputs: (rc, outputs)"""
    T, Cn = beta.shape
    lad = np.ascontiguousarray(ladder, np.int32)
    outs = [np.full((T, max(K, 1)), -7, np.int32), np.full((T, Cn), -7, np.int32), np.full((Cn, max(R, 1)), -7, np.int64),
            np.full(Cn, -7, np.int64), np.full(max(K, 1), -7, np.int64)]
    rc = engine._L.bh_chain_ladder_index(engine._h, E.HOST, None, T, Cn, Cn, E._ptr(beta), E._ptr(lad), K, R, E._ptr(outs[0]), max(K, 1),
                                         E._ptr(outs[1]), Cn, E._ptr(outs[2]), E._ptr(outs[3]), E._ptr(outs[4]))
    return rc, outs


def test_ladder_index_refusals_leave_the_outputs_untouched(engine):
    import torch
    rs = np.random.RandomState(3)
    ladder = [0] * 4 + [1] * 4
    beta = LR.permuted_betas(rs, 9, ladder)
    rc, outs = raw_index(engine, beta, ladder, 2, 4)
    assert rc == E.BH_OK and not any(np.any(o == -7) for o in outs)
    many = LR.permuted_betas(rs, 3, [0] * 65)
    rc, outs = raw_index(engine, many, [0] * 65, 1, 65)
    assert rc == E.BH_EUNSUPPORTED and all(np.all(o == -7) for o in outs)
    rc, outs = raw_index(engine, LR.permuted_betas(rs, 3, [0] * 64), [0] * 64, 1, 64)
    assert rc == E.BH_OK
    cases = []
    for v in (np.nan, np.inf, -np.inf):
        b = beta.copy()
        b[5, 6] = v
        cases.append(("beta %r" % v, dict(beta=b, ladder=ladder, K=2, R=4)))
    cases += [("an unused id", dict(beta=beta, ladder=[0] * 4 + [2] * 4, K=3, R=4)), ("an id beyond K", dict(beta=beta, ladder=[0] * 4 + [2] * 4, K=2, R=4)),
              ("a negative id", dict(beta=beta, ladder=[0] * 4 + [-1] * 4, K=2, R=4)), ("R too small", dict(beta=beta, ladder=ladder, K=2, R=3)),
              ("K = 0", dict(beta=beta, ladder=ladder, K=0, R=4))]
    for what, kw in cases:
        rc, outs = raw_index(engine, **kw)
        assert rc == E.BH_EINVAL, what
        assert all(np.all(o == -7) for o in outs), what
    with pytest.raises(E.EngineError, match="finite"):
        b = torch.from_numpy(beta).to(torch.device("cuda", 0))
        b[8, 0] = float("nan")
        D.ladder_index(b, ladder, engine=engine)
    with pytest.raises(E.EngineError, match="BH_LADDER_MAXRUNGS"):
        D.ladder_index(many, [0] * 65, engine=engine)


# ---- gathered sums ----------------------------------------------------------------------------------------------------------------
def make_table(seed, T, Cn, Q, dtype):
    """[T][C][Q] (the table of tests/test_gpu_chain_diag.py): column 0 like a likelihood series, the last column of Q >= 3 constant,
    the rest of mixed scale and sign"""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((T, Cn, Q)) * (10.0 ** rs.randint(-3, 4, size=(1, Cn, Q)))
    x[:, :, 0] = -1e4 + rs.standard_normal((T, Cn))
    if Q >= 3:
        x[:, :, Q - 1] = rs.standard_normal((1, 1)) * 100.0       # (constant along the gathered series too: the same in every chain)
    return x.astype(dtype)


def strided(x):
    """x inside a larger array of NaN: another ld_t, ld_c > Q, an offset; the gaps must never be read"""
    T, Cn, Q = x.shape
    big = np.full((2 * T + 1, Cn + 2, Q + 3), np.nan, x.dtype)
    view = big[1:2 * T + 1:2, 1:Cn + 1, 2:Q + 2]
    view[...] = x
    return big, (slice(1, 2 * T + 1, 2), slice(1, Cn + 1), slice(2, Q + 2))


def wide_sel(sel):
    """sel as a view with ld_sel > K, between columns of out-of-range indices that must never be read"""
    big = np.full((sel.shape[0], sel.shape[1] + 3), 1 << 30, np.int32)
    big[:, 2:2 + sel.shape[1]] = sel
    return big[:, 2:2 + sel.shape[1]]


def mask_unselected(x, sel):
    """a copy of x with every element of a chain that is not selected at a row a NaN"""
    keep = np.zeros(x.shape[:2], bool)
    keep[np.arange(x.shape[0])[:, None], sel] = True
    y = x.copy()
    y[~keep] = np.nan
    return y


def selections(rs, T, Cn, K):
    """random per row (it switches inside tiles and halos), constant, and one in which two series share a chain at some rows"""
    rnd = np.stack([rs.permutation(Cn)[:K] for _ in range(T)]).astype(np.int32)
    const = np.tile(rs.permutation(Cn)[:K].astype(np.int32), (T, 1))
    shared = rnd.copy()
    if K > 1:
        shared[::3, 1] = shared[::3, 0]
    else:
        shared[:] = Cn - 1
    return dict(random=rnd, constant=const, shared=shared)


def same(a, b):
    return all(np.array_equal(a[k], b[k]) and not np.any(np.signbit(a[k]) != np.signbit(b[k])) for k in KEYS) and \
        a["T"] == b["T"] and a["maxlag"] == b["maxlag"]


def check_series(col, out, L, k, q):
    """the returned sums of series (k, q) against their exact values, each within n * 2^-53 * sum |terms| (tests/diag_ref.py)"""
    T = col.shape[0]
    r1 = R.pass1(col)
    assert out["x0"][k, q] == r1["x0"]
    for key in ("s1", "s1a", "s1b"):
        val, bound = r1[key]
        assert abs(out[key][k, q] - val) <= bound, (key, k, q, out[key][k, q], val, bound)
    m, ma, mb = R.means(T, out["s1"][k, q], out["s1a"][k, q], out["s1b"][k, q])
    r2 = R.pass2(r1["d"], m, ma, mb, L)
    for key in ("m2a", "m2b"):
        val, bound = r2[key]
        assert abs(out[key][k, q] - val) <= bound, (key, k, q, out[key][k, q], val, bound)
    for lag, (val, bound) in enumerate(r2["p"]):
        assert abs(out["p"][k, q, lag] - val) <= bound, ("p", lag, k, q, out["p"][k, q, lag], val, bound)


# (T, L) of tests/test_gpu_chain_diag.py::CASES: T in {1, 2, 3, 7, tile-1, tile, tile+1, 2 tile + 68, 2 tile + 1033, MAXLAG + 2},
# L in {0, 1, 63, 64, 65, T-1, T, T+5, 1030, MAXLAG}; C = 5 chains; (K, Q) goes through {1, 3} x {1, 3, 64} along the list, every
# pair at least twice, and the pairs move on by one for the other dtype
SHAPES = [(1, 0), (1, 6), (2, 1), (3, 3), (7, 6), (7, 12), (7, 3), (TILE - 1, 63), (TILE, 64), (TILE + 1, 65), (TILE + 1, 0),
          (2 * TILE + 65 + 3, 65), (2 * TILE + 1030 + 3, 1030), (MAXLAG + 2, MAXLAG)]
KQ = [(1, 1), (3, 3), (1, 64), (3, 1), (1, 3), (3, 64)]
CASES = [(T, L, i) for i, (T, L) in enumerate(SHAPES)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("T,L,i", CASES)
def test_gathered_sums_have_the_bits_of_the_gathered_table(engine, T, L, i, dtype):
    """Expected: chain_series_stats of np.take_along_axis(x, sel, 1) -- the call without a selection, itself held to tests/diag_ref.py
    by tests/test_gpu_chain_diag.py; four series per case also directly against diag_ref within the summation bounds.  A host table,
    a strided host view, a device tensor and a strided device view, and a selection with ld_sel > K, give the same bits."""
    import torch
    K, Q = KQ[(i + (dtype == np.float64)) % len(KQ)]
    rs = np.random.RandomState(T * 1000 + L)
    x = make_table(T * 1000 + L, T, NCHAINS, Q, dtype)
    dev = torch.device("cuda", 0)
    for kind, sel in selections(rs, T, NCHAINS, K).items():
        gathered = np.take_along_axis(x, sel[:, :, None].astype(np.int64), 1)
        want = D.chain_series_stats(gathered, L, engine=engine)
        y = mask_unselected(x, sel)
        assert np.isnan(y).any() or K == NCHAINS
        got = D.chain_series_stats(y, L, engine=engine, sel=sel)
        assert got["p"].shape == (K, Q, L + 1) and got["x0"].shape == (K, Q) and got["T"] == T and got["maxlag"] == L
        assert same(want, got), kind
        if kind != "random":
            assert same(want, D.chain_series_stats(torch.from_numpy(y).to(dev), L, engine=engine, sel=torch.from_numpy(sel).to(dev))), kind
            continue
        picks = sorted(set([(0, 0), (K - 1, Q - 1), (0, Q - 1), (K - 1, Q // 2)]))
        for k, q in picks:
            check_series(gathered[:, k, q], got, L, k, q)
        big, sl = strided(y)
        assert same(want, D.chain_series_stats(big[sl], L, engine=engine, sel=wide_sel(sel)))
        tsel = torch.from_numpy(sel).to(dev)
        assert same(want, D.chain_series_stats(torch.from_numpy(y).to(dev), L, engine=engine, sel=tsel))
        tbig = torch.from_numpy(big).to(dev)
        view = tbig[sl]
        wsel = torch.from_numpy(np.ascontiguousarray(wide_sel(sel).base)).to(dev)[:, 2:2 + K]
        assert view.data_ptr() != tbig.data_ptr() and (K == 1 or T == 1 or wsel.stride(0) == K + 3)
        assert same(want, D.chain_series_stats(view, L, engine=engine, sel=wsel))
        if Q == 1:     # the [T][C] form of likes and vpvs
            assert same(want, D.chain_series_stats(torch.from_numpy(y[:, :, 0].copy()).to(dev), L, engine=engine, sel=tsel))


def test_wide_tables_take_several_gathered_calls(engine):
    T, L, K, Q = 40, 9, 3, 70
    rs = np.random.RandomState(8)
    x = make_table(8, T, NCHAINS, Q, np.float32)
    sel = selections(rs, T, NCHAINS, K)["random"]
    want = D.chain_series_stats(np.take_along_axis(x, sel[:, :, None].astype(np.int64), 1), L, engine=engine)
    assert same(want, D.chain_series_stats(mask_unselected(x, sel), L, engine=engine, sel=sel))


# ---- gathered model series --------------------------------------------------------------------------------------------------------
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
@pytest.mark.parametrize("ML,T,K,L", [(6, 37, 3, 20), (32, 70, 2, 8)])
def test_gathered_model_series_have_the_bits_of_the_gathered_rows(engine, ML, T, K, L, dtype):
    """every row of a chain that is not selected is malformed (an odd count): reading one is BH_EINVAL"""
    import torch
    rs = np.random.RandomState(ML)
    rows = model_rows(ML, T, NCHAINS, ML, dtype)
    dep = np.concatenate((np.arange(0, 60, 1.0), [60.125, 75.5, 200.0]))
    dev = torch.device("cuda", 0)
    for kind, sel in selections(rs, T, NCHAINS, K).items():
        want = D.chain_model_stats(np.take_along_axis(rows, sel[:, :, None].astype(np.int64), 1), dep, L, engine=engine)
        keep = np.zeros((T, NCHAINS), bool)
        keep[np.arange(T)[:, None], sel] = True
        y = rows.copy()
        y[~keep] = np.nan
        y[~keep, :3] = 1.0
        with pytest.raises(E.EngineError, match="prefix of even length"):
            D.chain_model_stats(y, dep, L, engine=engine)
        got = D.chain_model_stats(y, dep, L, engine=engine, sel=sel)
        assert got["x0"].shape == (K, dep.size + 1) and same(want, got), kind
        assert same(want, D.chain_model_stats(torch.from_numpy(y).to(dev), dep, L, engine=engine, sel=torch.from_numpy(sel).to(dev))), kind
        big = np.full((T + 1, NCHAINS + 1, 2 * ML + 2), np.nan, dtype)
        big[1:, :NCHAINS, :2 * ML] = y
        wsel = torch.from_numpy(np.ascontiguousarray(wide_sel(sel).base)).to(dev)[:, 2:2 + K]
        assert same(want, D.chain_model_stats(torch.from_numpy(big).to(dev)[1:, :NCHAINS, :2 * ML], dep, L, engine=engine, sel=wsel)), kind
        few = D.chain_model_stats(y, dep[:0], L, engine=engine, sel=sel)          # no depths: nlayers alone
        assert all(np.array_equal(few[k][:, 0], want[k][:, -1]) for k in KEYS)


# ---- gathered medians -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("T", [1, 2, 3, 100, 1001])
def test_gathered_medians_are_numpys_bits(engine, T, dtype):
    import torch
    rs = np.random.RandomState(T)
    K = 3
    x = (rs.standard_normal((T, NCHAINS)) * 10.0 ** rs.randint(-2, 3, size=(1, NCHAINS))).astype(dtype)
    x[:, 1] = np.round(x[:, 1])                 # ties
    x[:, 2] = -np.abs(x[:, 2]) - 1e4            # all negative
    dev = torch.device("cuda", 0)
    for kind, sel in selections(rs, T, NCHAINS, K).items():
        want = np.median(np.take_along_axis(x, sel.astype(np.int64), 1), axis=0)
        assert want.dtype == dtype
        y = mask_unselected(x, sel)
        got = D.chain_medians(torch.from_numpy(y).to(dev), engine=engine, sel=torch.from_numpy(sel).to(dev))
        assert got.dtype == dtype and np.array_equal(got, want), kind
        assert np.array_equal(D.chain_medians(y, sel=sel), want)           # (numpy: np.median of the gathered column)
        big = np.full((T + 2, NCHAINS + 3), np.nan, dtype)
        big[1:T + 1, 2:NCHAINS + 2] = y
        wsel = torch.from_numpy(np.ascontiguousarray(wide_sel(sel).base)).to(dev)[:, 2:2 + K]
        assert np.array_equal(D.chain_medians(torch.from_numpy(big).to(dev)[1:T + 1, 2:NCHAINS + 2], engine=engine, sel=wsel), want), kind
        # the host memspace of the engine call
        lo, hi = np.full(K, FILL), np.full(K, FILL)
        rc = engine._L.bh_chain_diag_medians_sel(engine._h, E.HOST, None, y.itemsize, T, NCHAINS, NCHAINS, 1, E._ptr(y), K, E._ptr(sel), K,
                                                 E._ptr(lo), E._ptr(hi))
        assert rc == E.BH_OK
        ranked = np.sort(np.take_along_axis(x, sel.astype(np.int64), 1), axis=0)
        assert np.array_equal(ranked[(T - 1) // 2], lo.astype(dtype)) and np.array_equal(ranked[T // 2], hi.astype(dtype)), kind


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def raw_sel_call(engine, big, sl, sel, L, K=None, ld_sel=None, what="series", dep=None):
    """the gathered engine calls on the host view big[sl] (inside its NaN-filled allocation) with prefilled outputs: (rc, outputs)"""
    view = big[sl]
    T, Cn, W = view.shape
    K = sel.shape[1] if K is None else K
    ld_sel = sel.shape[1] if ld_sel is None else ld_sel
    ld_t, ld_c = view.strides[0] // view.itemsize, view.strides[1] // view.itemsize
    ptr = C.c_void_p(view.ctypes.data)
    nk = max(K, 1)
    if what == "medians":
        outs = [np.full(nk, FILL), np.full(nk, FILL)]
        rc = engine._L.bh_chain_diag_medians_sel(engine._h, E.HOST, None, view.itemsize, T, Cn, ld_t, ld_c, ptr, K, E._ptr(sel), ld_sel,
                                                 *[E._ptr(o) for o in outs])
        return rc, outs
    nq = W if what == "series" else len(dep) + 1
    outs = [np.full((nk, nq), FILL) for _ in D.FIELDS] + [np.full((nk, nq, L + 1), FILL)]
    if what == "series":
        rc = engine._L.bh_chain_diag_series_sel(engine._h, E.HOST, None, view.itemsize, T, Cn, W, ld_t, ld_c, ptr, K, E._ptr(sel), ld_sel, L,
                                                *[E._ptr(o) for o in outs])
    else:
        d = np.ascontiguousarray(dep, np.float64)
        rc = engine._L.bh_chain_diag_models_sel(engine._h, E.HOST, None, view.itemsize, T, Cn, W // 2, ld_t, ld_c, ptr, K, E._ptr(sel), ld_sel,
                                                len(d), E._ptr(d), L, *[E._ptr(o) for o in outs])
    return rc, outs


def test_gathered_refusals_leave_the_outputs_untouched(engine):
    """indices -1 and C: the table lies inside a larger NaN-filled allocation, so even an unchecked read would stay inside the buffer"""
    import torch
    T, K, L = 20, 2, 4
    rs = np.random.RandomState(11)
    x = make_table(11, T, NCHAINS, 3, np.float64)
    sel = selections(rs, T, NCHAINS, K)["random"]
    big, sl = strided(x)
    rc, outs = raw_sel_call(engine, big, sl, sel, L)
    assert rc == E.BH_OK and not any(np.any(o == FILL) for o in outs)
    rows = model_rows(2, T, NCHAINS, 4, np.float32)
    mbig, msl = strided(rows)
    assert raw_sel_call(engine, mbig, msl, sel, L, what="models", dep=[1.0, 2.0])[0] == E.BH_OK
    lbig, lsl = strided(x[:, :, :1])
    assert raw_sel_call(engine, lbig, lsl, sel, L, what="medians")[0] == E.BH_OK
    for bad in (-1, NCHAINS, 1 << 30, -(1 << 31)):
        for where in ((0, 0), (T - 1, K - 1), (7, 1)):
            s = sel.copy()
            s[where] = bad
            for what, b, l, kw in (("series", big, sl, {}), ("models", mbig, msl, dict(dep=[1.0, 2.0])), ("medians", lbig, lsl, {})):
                rc, outs = raw_sel_call(engine, b, l, s, L, what=what, **kw)
                assert rc == E.BH_EINVAL, (bad, where, what)
                assert "index" in engine._L.bh_engine_last_error(engine._h).decode(), (bad, where, what)
                assert all(np.all(o == FILL) for o in outs), (bad, where, what)
    for what, kw in (("K = 0", dict(K=0)), ("K < 0", dict(K=-1)), ("ld_sel < K", dict(ld_sel=K - 1))):
        for call, b, l, extra in (("series", big, sl, {}), ("models", mbig, msl, dict(dep=[1.0, 2.0])), ("medians", lbig, lsl, {})):
            rc, outs = raw_sel_call(engine, b, l, sel, L, what=call, **dict(kw, **extra))
            assert rc == E.BH_EINVAL, (what, call)
            assert all(np.all(o == FILL) for o in outs), (what, call)
    dev = torch.device("cuda", 0)
    s = sel.copy()
    s[3, 0] = NCHAINS
    tbig = torch.from_numpy(big).to(dev)
    with pytest.raises(E.EngineError, match="index"):
        D.chain_series_stats(tbig[sl], L, engine=engine, sel=torch.from_numpy(s).to(dev))
    with pytest.raises(E.EngineError, match="index"):
        D.chain_medians(tbig[sl][:, :, 0], engine=engine, sel=torch.from_numpy(s).to(dev))
    with pytest.raises(E.EngineError, match="finite"):      # a selected NaN is still a value that is not finite
        y = x.copy()
        y[5, sel[5, 1], 2] = np.nan
        D.chain_series_stats(y, L, engine=engine, sel=sel)
    with pytest.raises(ValueError):
        D.chain_series_stats(x, L, engine=engine, sel=sel[:-1])
    with pytest.raises(ValueError):
        D.chain_series_stats(x, L, engine=engine, sel=torch.from_numpy(sel).to(dev))      # a numpy table wants a numpy selection


# ---- a tempered run end to end ----------------------------------------------------------------------------------------------------
def same_result(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        if isinstance(a[k], dict):
            same_result(a[k], b[k], what + (k,))
        else:
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert x.shape == y.shape and np.array_equal(x, y, equal_nan=(x.dtype.kind == "f")), what + (k,)


OWN = ("outlier_chains", "ladders")      # what ladder_diagnostics adds to the dict of diagnose


def check_ladders(lad, beta, ladder, chains, T):
    """the `ladders` entry of a site against the restatement applied to the recorded betas of the site's chains"""
    want = LR.ladder_index(beta[:, chains], np.asarray(ladder)[chains])
    assert np.array_equal(lad["ids"], want["ids"]) and np.array_equal(lad["moves"], want["moves"])
    assert len(lad["members"]) == len(want["members"]) and all(np.array_equal(a, chains[b]) for a, b in zip(lad["members"], want["members"]))
    assert np.array_equal(lad["chains"], chains) and np.array_equal(lad["round_trips"], want["round_trips"])
    assert np.array_equal(lad["occupancy"], want["occupancy"]) and np.all(lad["occupancy"].sum(axis=1) == T)
    assert np.array_equal(lad["cold_share"], want["occupancy"][:, 0] / float(T))


@pytest.fixture(scope="module")
def tempered_run(tmp_path_factory):
    """the tempered set-up of tests/test_gpu_chain_record.py -- two ladders of four temperatures, exchanges every 20 iterations, seed 5,
    recorded on the device -- with a main phase of 400 iterations thinned to 100 rows: 20 exchange sweeps fall into the diagnosed phase"""
    from test_gpu_chains import SETUPS, make_targets
    g = golden("chain_golden.npz")
    su = SETUPS["exp"]
    init = dict(su["init"], iter_burnin=280, iter_main=400, maxmodels=100, savepath=str(tmp_path_factory.mktemp("ladders")))
    ladder = np.repeat(np.arange(2), 4)
    betas = np.tile(1.0 / np.geomspace(1.0, 20.0, 4), 2)
    return DeviceChains(make_targets(g), 8, init, su["priors"], seed=5, betas=betas, ladder=ladder, swap_every=20, record="device").run()


def test_ladder_diagnostics_of_a_tempered_run(tempered_run):
    dev = tempered_run
    diag = dev.ladder_diagnostics()
    h = dev.samples("p2", cold_only=True)
    T = h["likes"].shape[0]
    assert dev.thinning == 4 and T == 100 and dev.nswaps > 0
    assert diag["ladders"]["moves"].sum() > 0        # the cold state moved between chains inside the diagnosed phase
    assert diag["maxlag"] == min(T // 2, 1000) and np.array_equal(diag["dep"], np.linspace(0, 100, 41))
    assert list(h["ladder"]) == [0, 1]
    # the same calls on the cold series gathered on the host: the same kernels on the same values
    host = D.diagnose(h, np.zeros(2, int), h["ladder"], engine=dev.engine)[0]
    same_result({k: v for k, v in diag.items() if k not in OWN}, host, ("host",))
    stored = results.diagnostics_from_storage([dev.save()], engine=dev.engine)[0]
    for k in D.GROUPS:
        same_result(diag[k], stored[k], ("stored", k))
    assert np.array_equal(diag["outliers"], stored["outliers"]) and np.array_equal(diag["scores"], stored["scores"])
    assert set(diag["likes"]["chains"]) == {0, 1} - set(diag["outliers"]) and np.array_equal(diag["chain_ids"], [0, 1])
    members = [m for lid, m in zip(diag["ladders"]["ids"], diag["ladders"]["members"]) if lid in diag["outliers"]]
    assert np.array_equal(diag["outlier_chains"], np.concatenate(members) if members else np.zeros(0, np.int64))
    ps = dev.posterior_scalars(exclude_chains=diag["outlier_chains"])
    assert isinstance(ps, dict)
    full = dev.samples("p2")
    check_ladders(diag["ladders"], full["beta"], dev.ladder, np.arange(8), T)
    assert np.all(diag["ladders"]["cold_share"] >= 0) and abs(diag["ladders"]["cold_share"].sum() - 2.0) < 1e-12
    # a sequence of ladder ids overrides the outliers; other lag and depths; the burn-in phase
    over = dev.ladder_diagnostics(exclude_ladders=[1], maxlag=5, dep=[1.0, 30.0])
    assert list(over["likes"]["chains"]) == [0] and over["vs"]["rhat"].shape == (2,) and over["maxlag"] == 5
    assert np.array_equal(over["outliers"], diag["outliers"])
    p1 = dev.ladder_diagnostics("p1")
    h1 = dev.samples("p1", cold_only=True)
    same_result({k: v for k, v in p1.items() if k not in OWN}, D.diagnose(h1, np.zeros(2, int), h1["ladder"], engine=dev.engine)[0], ("p1",))
    check_ladders(p1["ladders"], dev.samples("p1")["beta"], dev.ladder, np.arange(8), h1["likes"].shape[0])
    with pytest.raises(E.EngineError, match="tempered"):      # per-chain diagnostics of a tempered run stay meaningless
        dev.diagnostics()


def test_ladder_diagnostics_of_many_sites():
    """2 sites x 2 ladders x 2 temperatures: one dict per site with the site's own ladder ids"""
    from test_gpu_sites_priors import SITE_INIT, SITE_PRIORS, full_site
    g = golden("chain_golden.npz")
    st = bh.SiteTargets([full_site(g, s, "phase_rf") for s in range(2)], names=["st0", "st1"], per_site_x="all", per_site_rf=True)
    inits = [dict(SITE_INIT[s], iter_burnin=80, iter_main=200, maxmodels=50) for s in range(2)]
    ladder = np.array([10, 10, 11, 11, 12, 12, 13, 13])
    betas = np.tile([1.0, 0.25], 4)
    dev = DeviceChains(st, 4, inits, SITE_PRIORS[:2], seed=77, search="fast", betas=betas, ladder=ladder, swap_every=10, record="device").run()
    diag = dev.ladder_diagnostics()
    assert len(diag) == 2
    full = dev.samples("p2")
    T = full["likes"].shape[0]
    assert T >= 16
    for s in range(2):
        h = dev.samples("p2", cold_only=True, site=s)
        ids = [10 + 2 * s, 11 + 2 * s]
        assert list(h["ladder"]) == ids and list(diag[s]["chain_ids"]) == ids and list(diag[s]["ladders"]["ids"]) == ids
        check_ladders(diag[s]["ladders"], full["beta"], ladder, np.arange(4 * s, 4 * s + 4), T)
        assert set(diag[s]["likes"]["chains"]) | set(diag[s]["outliers"]) == set(ids)
        assert set(diag[s]["outlier_chains"]) == {c for c in range(8) if ladder[c] in diag[s]["outliers"]}
    # the sums of every site's cold series: those of the call without a selection on the series gathered on the host
    hall = dev.samples("p2", cold_only=True)
    host = D.diagnose(hall, np.array([0, 0, 1, 1]), hall["ladder"], engine=dev.engine)
    for s in range(2):
        same_result({k: v for k, v in diag[s].items() if k not in OWN}, host[s], (s, "host"))


def test_ladder_diagnostics_refuses_untempered_runs_and_host_records():
    from test_gpu_chains import SETUPS, make_targets
    g = golden("chain_golden.npz")
    su = SETUPS["exp"]
    init = dict(su["init"], iter_burnin=280, iter_main=60, maxmodels=15)
    plain = DeviceChains(make_targets(g), 4, init, su["priors"], seed=5, record="device")
    with pytest.raises(E.EngineError, match="untempered"):
        plain.ladder_diagnostics()
    ladder = np.repeat(np.arange(2), 2)
    betas = np.tile([1.0, 0.2], 2)
    host = DeviceChains(make_targets(g), 4, init, su["priors"], seed=5, betas=betas, ladder=ladder, swap_every=20, record="host")
    with pytest.raises(E.EngineError, match="record='device'"):
        host.ladder_diagnostics()
