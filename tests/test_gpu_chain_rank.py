"""The rank transform on the GPU (include/bh_engine_chain_rank.h, bayhunter_amd/diagnostics.py): z, zf and tail bit for bit against
the restatement tests/rank_ref.py -- every output is a function of integer counts and of one table lookup, so there is no
tolerance --, their stability, the model-row series, the numbers downstream, the refusals, and a recorded run end to end."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import diag_ref as R
import rank_ref as K
from conftest import REPO
from bayhunter_amd import diagnostics as D
from bayhunter_amd import engine as E
from bayhunter_amd import results
from bayhunter_amd.posterior import stepmodel
from test_gpu_chain_diag import model_rows, same_result, site_run, strided  # noqa: F401  (site_run: the recorded run's fixture)

pytestmark = pytest.mark.gpu

NAMES = ("z", "zf", "tail")


def test_python_constants_mirror_the_header():
    txt = open(os.path.join(REPO, "include", "bh_engine_chain_rank.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define\s+(BH_RANK_[A-Z]+)\s+(\d+)\b", txt, flags=re.M)}
    assert defs == {"BH_RANK_TILE": E.RANK_TILE, "BH_RANK_RADIXBITS": E.RANK_RADIXBITS} and (E.RANK_TILE, E.RANK_RADIXBITS) == (4096, 8)
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert sorted(set(re.findall(r"\b(bh_[a-z_]+)\s*\(", txt))) == sorted(E.CHAIN_RANK_SYMBOLS)
    lib = C.CDLL(E.LIB_PATH)
    assert all(hasattr(lib, n) for n in E.CHAIN_RANK_SYMBOLS) and lib.bh_abi_version() == 10


KINDS = 6


def column(rs, kind, shape, dtype):
    """one column [T][C] of the kind: 0 normal draws, 1 three distinct integers (long tie runs), 2 a constant, 3 both zeros, denormals
    and negative values, 4 values that differ only in the lowest mantissa bits and in the top exponent bits (every radix digit
    matters), 5 float32 values (in a float64 table: the ranks of the float32 table)"""
    f32 = dtype == np.float32
    if kind == 0:
        v = rs.standard_normal(shape) * 10.0 ** rs.randint(-3, 4)
    elif kind == 1:
        v = rs.randint(3, 6, shape).astype(np.float64)
    elif kind == 2:
        v = np.full(shape, -1234.5)
    elif kind == 3:
        tiny = 1e-40 if f32 else 1e-310
        v = rs.choice(np.array([-0.0, 0.0, tiny, -tiny, 3 * tiny, -2.5, -1e-3, 1.0]), shape)
    elif kind == 4:
        ulp, es = (2.0 ** -23, (-120, -60, 0, 60, 120)) if f32 else (2.0 ** -52, (-1000, -500, 0, 500, 1000))
        v = (1.0 + rs.randint(0, 4, shape) * ulp) * 2.0 ** rs.choice(np.array(es, dtype=np.float64), shape) * rs.choice([-1.0, 1.0], shape)
    else:
        v = rs.standard_normal(shape).astype(np.float32).astype(np.float64)
    return v.astype(dtype)


def make_table(seed, T, Cn, Q, dtype, first=0):
    """[T][C][Q], column q of kind (first + q) % KINDS"""
    rs = np.random.RandomState(seed)
    x = np.empty((T, Cn, Q), dtype)
    for q in range(Q):
        x[:, :, q] = column(rs, (first + q) % KINDS, (T, Cn), dtype)
    if Q > 3:
        assert np.any(np.signbit(x) & (x == 0)) and np.any(~np.signbit(x) & (x == 0))
    return x


def same_bits(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        g = g.cpu().numpy() if hasattr(g, "cpu") else np.asarray(g)
        w = np.asarray(w).reshape(g.shape)
        assert g.dtype == w.dtype and np.array_equal(g, w) and not np.any(np.signbit(g) != np.signbit(w)), what + (name,)


# (T, C, Q, group): a pool of one; two chains; interleaved sites with a chain left out in the middle; 4098 elements in one pool --
# across the sort tiles, a remainder of 2; the column limit with pools of 1, 2 and 4 chains
CASES = [(1, 1, 1, [0]), (4, 2, 1, [0, 0]), (37, 5, 3, [1, 0, -1, 0, 1]), (1366, 3, 2, [0, 0, 0]),
         (300, 7, 64, [2, 1, 2, 0, 2, 1, 2])]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("T,Cn,Q,group", CASES)
def test_rank_tables_are_the_restatements_bits(engine, T, Cn, Q, group, dtype):
    """every kind of column at every shape; a contiguous table and the strided view, from host and from device memory"""
    import torch
    dev = torch.device("cuda", 0)
    for first in (range(0, KINDS, Q) if Q < KINDS else [0]):
        x = make_table(1000 * T + first, T, Cn, Q, dtype, first)
        want = K.rank_tables(x, group)
        big, sl = strided(x)
        same_bits(D.rank_series(x, group, engine=engine), want, (first, "host"))
        same_bits(D.rank_series(big[sl], group, engine=engine), want, (first, "host view"))
        same_bits(D.rank_series(torch.from_numpy(x).to(dev), group, engine=engine), want, (first, "device"))
        tbig = torch.from_numpy(big).to(dev)
        got = D.rank_series(tbig[sl], group, engine=engine)
        assert tbig[sl].data_ptr() != tbig.data_ptr() and all(g.is_cuda for g in got)
        same_bits(got, want, (first, "device view"))
        left = [c for c in range(Cn) if group[c] < 0]
        assert all(not np.any(w[:, left]) for w in want) and all(not bool(g[:, left].any()) for g in got)
    if Q == 1:          # the [T][C] form of likes and vpvs
        z, zf, tail = D.rank_series(torch.from_numpy(x[:, :, 0].copy()).to(dev), group, engine=engine)
        assert z.shape == (T, Cn) and zf.shape == (T, Cn) and tail.shape == (T, Cn, 2)
        same_bits((z, zf, tail), want, ("2-D",))


def test_a_float64_table_of_float32_values_has_the_float32_tables_ranks(engine):
    """the 32-bit keys of a float32 table and the 64-bit keys of the same values order alike"""
    import torch
    x32 = make_table(77, 1366, 3, 6, np.float32)
    group = [0, 0, 0]
    a = D.rank_series(torch.from_numpy(x32).cuda(), group, engine=engine)
    b = D.rank_series(torch.from_numpy(x32.astype(np.float64)).cuda(), group, engine=engine)
    same_bits(a, [t.cpu().numpy() for t in b], ("float32 / float64",))
    same_bits(a, K.rank_tables(x32, group), ("restatement",))


def test_a_pool_has_the_same_bits_alone_and_among_others(engine):
    import torch
    T, Cn, Q = 300, 7, 5
    group = np.array([2, 1, 2, 0, 2, 1, 2])
    x = make_table(5, T, Cn, Q, np.float64, first=3)
    dev = torch.device("cuda", 0)
    among = [t.cpu().numpy() for t in D.rank_series(torch.from_numpy(x).to(dev), group, engine=engine)]
    again = D.rank_series(torch.from_numpy(x).to(dev), group, engine=engine)
    same_bits(again, among, ("repeat",))
    same_bits(D.rank_series(x, group, engine=engine), among, ("host",))
    big, sl = strided(x)
    same_bits(D.rank_series(torch.from_numpy(big).to(dev)[sl], group, engine=engine), among, ("other leading dimensions",))
    for g, q in ((1, 2), (0, 0), (2, 4)):
        cs = np.flatnonzero(group == g)
        alone = D.rank_series(torch.from_numpy(x[:, cs, q:q + 1].copy()).to(dev), np.zeros(cs.size, int), engine=engine)
        want = (among[0][:, cs, q:q + 1], among[1][:, cs, q:q + 1], among[2][:, cs, 2 * q:2 * q + 2])
        same_bits(alone, want, ("alone", g, q))
    # without the fold or the tail the others do not change
    z, zf, tail = D.rank_series(x, group, engine=engine, folded=False)
    assert zf is None
    same_bits((z, among[1], tail), among, ("folded=False",))
    z, zf, tail = D.rank_series(x, group, engine=engine, tail=False)
    assert tail is None
    same_bits((z, zf, among[2]), among, ("tail=False",))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("ML,T,Cn", [(6, 37, 3), (32, 70, 2)])
def test_model_ranks_equal_the_ranks_of_the_host_table(engine, ML, T, Cn, dtype):
    import torch
    rows = model_rows(ML, T, Cn, ML, dtype)
    dep = np.concatenate((np.arange(0, 60, 1.0), [60.125, 75.5, 200.0]))
    assert dep.size == E.DIAG_MAXDEPTHS
    table = np.zeros((T, Cn, dep.size + 1))
    for t in range(T):
        for c in range(Cn):
            vs_step, dep_step = stepmodel(rows[t, c])
            table[t, c, :-1] = np.interp(dep, dep_step, vs_step)
            table[t, c, -1] = vs_step.size // 2 - 1
    group = [0, 1, 0][:Cn] if Cn == 3 else [0, 0]
    want = D.rank_series(table, group, engine=engine)
    same_bits(want, K.rank_tables(table, group), ("restatement",))
    same_bits(D.rank_models(rows, dep, group, engine=engine), want, ("host",))
    dev = torch.device("cuda", 0)
    same_bits(D.rank_models(torch.from_numpy(rows).to(dev), dep, group, engine=engine), want, ("device",))
    big = np.full((T + 1, Cn + 1, 2 * ML + 2), np.nan, dtype)
    big[1:, :Cn, :2 * ML] = rows
    same_bits(D.rank_models(torch.from_numpy(big).to(dev)[1:, :Cn, :2 * ML], dep, group, engine=engine), want, ("device view",))
    D_ = dep.size
    last = D.rank_models(torch.from_numpy(rows).to(dev), dep, group, engine=engine, columns=(D_ - 1, 2))
    same_bits(last, (want[0][:, :, D_ - 1:], want[1][:, :, D_ - 1:], want[2][:, :, 2 * D_ - 2:]), ("columns",))
    few = D.rank_models(rows, dep[:0], group, engine=engine)          # no depths: nlayers alone
    same_bits(few, (want[0][:, :, D_:], want[1][:, :, D_:], want[2][:, :, 2 * D_:]), ("nlayers",))
    bad = rows.copy()
    bad[3, 1, 0] = np.nan                                             # a gap before the values
    with pytest.raises(E.EngineError):
        D.rank_models(bad, dep, group, engine=engine)


def test_rank_convergence_of_device_tensors_equals_the_restatements(engine):
    """rank_convergence on a device tensor against convergence(chain_series_stats(.)) of the restatement's host tables, bit for
    bit, whatever the byte budget cuts the columns into"""
    import torch
    T, Cn, Q, L = 400, 6, 3, 60
    x = R.ar1(np.random.RandomState(424242), T, Cn, 0.7, Q)
    x[:, 1, 1] *= 3.0
    x[:, :, 2] = np.round(x[:, :, 2])
    site_of, exclude = np.array([0, 1, 0, 1, 0, 1]), (4,)
    group = np.where(np.arange(Cn) == 4, -1, site_of)
    conv = [D.convergence(D.chain_series_stats(t, L, engine=engine), site_of, exclude) for t in K.rank_tables(x, group)]
    want = [D.rank_summary(a, b, c) for a, b, c in zip(*conv)]
    tx = torch.from_numpy(x).cuda()
    for budget in (2 << 30, 1, 24 * T * Cn * 2):
        got = D.rank_convergence(tx, site_of, L, exclude, engine=engine, budget_bytes=budget)
        assert len(got) == 2
        for s in range(2):
            same_result(got[s], want[s], (budget, s))
    assert want[0]["chains"].tolist() == [0, 2] and want[1]["rhat_fold"][1] > want[1]["rhat_bulk"][1]
    host = D.rank_convergence(x.astype(np.float32), site_of, L, exclude, engine=engine)
    dev32 = D.rank_convergence(tx.to(torch.float32), site_of, L, exclude, engine=engine)
    for s in range(2):
        same_result(host[s], dev32[s], ("float32", s))


FILL = -7777.0


def raw_call(engine, x, group, G=None, Q=None, elem=None):
    """bh_chain_rank_series on a contiguous host table with prefilled outputs: (rc, outputs)"""
    T, Cn, W = x.shape
    Q = W if Q is None else Q
    group = np.ascontiguousarray(group, np.int32)
    G = int(group.max()) + 1 if G is None else G
    zt = D.rank_table(T * Cn)          # long enough for any pool of the table
    zoff = np.zeros(max(G, 1), np.int64)
    outs = [np.full((T, Cn, W), FILL), np.full((T, Cn, W), FILL), np.full((T, Cn, 2 * W), FILL, np.float32)]
    rc = engine._L.bh_chain_rank_series(engine._h, E.HOST, None, x.itemsize if elem is None else elem, T, Cn, Q, Cn * W, W, E._ptr(x),
                                        G, E._ptr(group), E._ptr(zt), E._ptr(zoff), *[E._ptr(o) for o in outs], Cn * W, W)
    return rc, outs


def test_refusals_leave_the_outputs_untouched(engine):
    import torch
    x = make_table(9, 20, 3, 3, np.float64)
    rc, outs = raw_call(engine, x, [0, 0, 0])
    assert rc == E.BH_OK and not any(np.any(o == FILL) for o in outs)
    wide = np.zeros((5, 1, 65))
    cases = []
    for v in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[13, 1, 2] = v
        cases.append(("value %r" % v, dict(x=y, group=[0, 0, 0])))
        cases.append(("value %r beside a chain left out" % v, dict(x=y, group=[-1, 0, 0])))
    cases += [("a group id of G", dict(x=x, group=[0, 2, 1], G=2)), ("a group id of -2", dict(x=x, group=[0, -2, 0], G=1)),
              ("an empty group", dict(x=x, group=[0, 0, 2])), ("no group", dict(x=x, group=[0, 0, 0], G=0)),
              ("Q = 65", dict(x=wide, group=[0])), ("elem_bytes 2", dict(x=x, group=[0, 0, 0], elem=2))]
    for what, kw in cases:
        rc, outs = raw_call(engine, **kw)
        assert rc == E.BH_EINVAL, what
        assert all(np.all(o == FILL) for o in outs), what
    # a device table and prefilled device outputs
    t = torch.from_numpy(x).cuda()
    t[19, 2, 0] = float("inf")
    douts = [torch.full((20, 3, 3), FILL, dtype=torch.float64).cuda(), torch.full((20, 3, 3), FILL, dtype=torch.float64).cuda(),
             torch.full((20, 3, 6), FILL, dtype=torch.float32).cuda()]
    group, zt, zoff = np.zeros(3, np.int32), D.rank_table(60), np.zeros(1, np.int64)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = engine._L.bh_chain_rank_series(engine._h, E.DEVICE, stream, 8, 20, 3, 3, 9, 3, C.c_void_p(t.data_ptr()), 1, E._ptr(group),
                                        E._ptr(zt), E._ptr(zoff), *[C.c_void_p(o.data_ptr()) for o in douts], 9, 3)
    torch.cuda.synchronize()
    assert rc == E.BH_EINVAL and all(bool((o == FILL).all()) for o in douts)
    with pytest.raises(E.EngineError):
        D.rank_series(t, [0, 0, 0], engine=engine)
    with pytest.raises(E.EngineError):
        D.rank_series(x, [0, 0, 2], engine=engine)
    # what is not finite in a chain that is left out is never read: accepted, and that chain's outputs are 0
    y = x.copy()
    y[:, 1, :] = np.nan
    y[3, 1, 1] = np.inf
    group = [0, -1, 0]
    want = K.rank_tables(np.where(np.isfinite(y), y, 0.0), group)
    for table in (y, torch.from_numpy(y).cuda()):
        got = D.rank_series(table, group, engine=engine)
        same_bits(got, want, ("NaN in a chain left out",))
        assert all(not bool(np.asarray(g.cpu() if hasattr(g, "cpu") else g)[:, 1].any()) for g in got)


CONV_KEYS = {"chains", "rhat", "ess", "tau", "cut", "ess_truncated", "constant", "mean", "std", "chain_tau"}


def strip(d):
    return {k: ({a: b for a, b in v.items() if a != "rank"} if isinstance(v, dict) else v) for k, v in d.items()}


def test_rank_diagnostics_of_a_recorded_run(site_run):
    dev = site_run
    plain = dev.diagnostics()
    diag = dev.diagnostics(rank=True)
    assert len(diag) == 2 and len(plain) == 2
    h = dev.samples("p2")
    host = D.diagnose(h, np.arange(8) // 4, np.arange(8), engine=dev.engine, rank=True)
    folders = dev.save()
    stored = results.diagnostics_from_storage(folders, engine=dev.engine, rank=True)
    nt = dev.nt
    for s in range(2):
        # without the flag: the keys and the bits of before, and nothing of the ranks
        assert set(plain[s]) == {"outliers", "scores", "chain_ids", "dep", "maxlag"} | set(D.GROUPS)
        assert all(set(plain[s][k]) == CONV_KEYS for k in D.GROUPS)
        same_result(plain[s], strip(diag[s]), (s, "rank stripped"))
        same_result(diag[s], host[s], (s, "host"))
        d, f = diag[s], stored[s]
        for k in D.GROUPS:
            same_result(d[k], f[k], (s, "stored", k))
            r = d[k]["rank"]
            assert set(r) == {"chains"} | set(D.RANK_FIELDS) and np.array_equal(r["chains"], d[k]["chains"])
        for k, width in (("likes", 1), ("vpvs", 1), ("misfits", nt + 1), ("noise", 2 * nt), ("vs", 41)):
            assert all(d[k]["rank"][a].shape == (width,) for a in D.RANK_FIELDS), k
        assert all(d["nlayers"]["rank"][a].shape == () for a in D.RANK_FIELDS)
        for k in ("likes", "vpvs", "misfits", "noise"):       # a column no kept chain moves in is constant in every rank table
            c, r = d[k]["constant"], d[k]["rank"]
            assert np.array_equal(r["constant_bulk"], c) and np.all(r["constant_fold"][c])
            assert np.all(np.isnan(r["rhat"][c])) and np.all(np.isnan(r["ess_bulk"][c])) and np.all(np.isnan(r["ess_tail"][c]))
            assert np.all(np.isfinite(r["rhat_bulk"][~c])) and np.all(r["ess_bulk"][~c] > 0)
            both = np.isfinite(r["rhat_fold"])
            assert np.array_equal(r["rhat"][both], np.maximum(r["rhat_bulk"], r["rhat_fold"])[both])
        assert np.isfinite(d["likes"]["rank"]["rhat"][0]) and d["likes"]["rank"]["ess_tail"][0] > 0
    over = dev.diagnostics(exclude_chains=[1, 6], maxlag=5, dep=[1.0, 30.0], rank=True)
    assert list(over[0]["likes"]["rank"]["chains"]) == [0, 2, 3] and list(over[1]["vs"]["rank"]["chains"]) == [4, 5, 7]
    assert over[0]["vs"]["rank"]["rhat"].shape == (2,)
    with pytest.raises(ValueError):
        dev.ladder_diagnostics(rank=True)
    with pytest.raises(ValueError):
        D.diagnose(h, np.arange(8) // 4, np.arange(8), engine=dev.engine, rank=True, sel=np.zeros((h["likes"].shape[0], 8), np.int32))
