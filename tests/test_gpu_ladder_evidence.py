"""The evidence estimates of tempered runs on the GPU (include/bh_engine_chain_ladder_evidence.h, bayhunter_amd/diagnostics.py:
ladder_holders, ladder_evidence): the holders, the extremes, the four sums and every derived number against the restatement
tests/evidence_ref.py, bit for bit, from host tables, device tables and strided device views inside NaN-filled allocations; the sums
against their values in extended precision; the invariances the header states; the refusals; a ladder whose evidence is known in
closed form; and DeviceChains.ladder_evidence of tempered runs end to end."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import evidence_ref as V
import ladder_ref as LR
from conftest import REPO, golden
import bayhunter_amd as bh
from bayhunter_amd import diagnostics as D
from bayhunter_amd import engine as E
from bayhunter_amd.device_chains import DeviceChains

pytestmark = pytest.mark.gpu

FILL = -7777.0
HEADER = "bh_engine_chain_ladder_evidence.h"
STATS = ("mean", "var", "tau", "ess", "rhat", "ess_truncated")
DERIVED = ("betas", "log_ratio", "log_ratio_rev", "ss", "ss_err", "ss_rev", "ss_rev_err", "ti", "ti2", "ti_err", "beta_min", "complete")


def test_python_constants_mirror_the_header():
    txt = open(os.path.join(REPO, "include", HEADER)).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define\s+(BH_EVIDENCE_[A-Z]+)\s+(\d+)\b", txt, flags=re.M)}
    assert defs == {"BH_EVIDENCE_DROP": E.EVIDENCE_DROP} and E.EVIDENCE_DROP == 512 == -V.DROP
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert sorted(set(re.findall(r"\b(bh_[a-z_]+)\s*\(", txt))) == sorted(E.CHAIN_LADDER_EVIDENCE_SYMBOLS)
    lib = C.CDLL(E.LIB_PATH)
    assert all(hasattr(lib, n) for n in E.CHAIN_LADDER_EVIDENCE_SYMBOLS) and lib.bh_abi_version() == 10
    assert not set(E.CHAIN_LADDER_EVIDENCE_SYMBOLS) & set(E.CHAIN_LADDER_SYMBOLS) and len(E.CHAIN_LADDER_SYMBOLS) == 4
    for hdr in sorted(os.listdir(os.path.join(REPO, "include"))):    # declared in the new header only
        if hdr != HEADER:
            other = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", hdr)).read(), flags=re.S)
            assert "bh_chain_ladder_holders" not in other and "bh_chain_ladder_evidence" not in other, hdr
    assert b"ev_sum_kernel" in open(E.LIB_PATH, "rb").read()
    assert D.EVIDENCE_SUMS == V.SUMS


# ---- the cases --------------------------------------------------------------------------------------------------------------------
SETS = {"one of 1": [7], "2, 5, 3 interleaved": [0, 1, 2, 1, 0, 1, 2, 1, 2, 1], "one of 64": [4] * 64}
TS = [1, 2, 15, 16, 17, 33, 257, 1000]
CONSTANT = {"one of 1": None, "2, 5, 3 interleaved": 4, "one of 64": 5}      # the series that is constant (2 + 2: rung 2 of ladder 1)


def make_case(T, which, dtype):
    """betas of ladder_ref.permuted_betas -- the ladder of two with betas 2^-40 apart instead --, likes in -6000 .. -5; one rung
    series constant; the hot series of the ladder of two steps by 2^-20, so that its forward terms take exp's 1 + x branch"""
    ladder = np.array(SETS[which])
    rs = np.random.RandomState(1000 * T + ladder.size)
    beta = LR.permuted_betas(rs, T, ladder)
    if ladder.size == 10:
        pair = np.flatnonzero(ladder == 0)
        beta[:, pair] = np.where(beta[:, pair] == 1.0, 1.0, 1.0 - 2.0 ** -40)
    likes = (-5.0 - rs.uniform(0.0, 5995.0, size=beta.shape)).astype(dtype)
    hold = V.holders(beta, ladder)[2]
    rows = np.arange(T)
    if ladder.size == 10:
        likes[rows, hold[:, 1]] = (-1.0 - 2.0 ** -20 * (rows % 8)).astype(dtype)
    if CONSTANT[which] is not None:
        likes[rows, hold[:, CONSTANT[which]]] = dtype(-777.0)
    return beta, likes, ladder


def package_stats(engine):
    """the numbers of the rung series by the package's existing calls on the table gathered on the host (no selection)"""
    def stats(gathered, L):
        tab = D.chain_series_stats(np.ascontiguousarray(gathered), L, engine=engine)
        conv = D.convergence(tab, np.arange(gathered.shape[1]))
        out = dict(mean=[c["mean"][0, 0] for c in conv], var=[tab["p"][j, 0, 0] / tab["T"] for j in range(len(conv))])
        for k in ("tau", "ess", "rhat", "ess_truncated"):
            out[k] = [c[k][0] for c in conv]
        return out
    return stats


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a.shape == b.shape and np.array_equal(a, b)


def same_evidence(got, want, what):
    assert bits(got["ids"], want["ids"]) and got["T"] == want["T"] and got["maxlag"] == want["maxlag"], what
    assert len(got["members"]) == len(want["members"]) and all(np.array_equal(a, b) for a, b in zip(got["members"], want["members"])), what
    g = host(got["hold"])
    assert g.dtype == np.int32 and np.array_equal(g, want["hold"]), (what, "hold")
    for k in ("rung_beta",) + V.SUMS:
        assert got[k].dtype == np.float64 and bits(got[k], want[k]), (what, k, got[k], want[k])
    assert len(got["ladders"]) == len(want["ladders"]), what
    for a, b in zip(got["ladders"], want["ladders"]):
        assert sorted(a) == sorted(b) == sorted(STATS + DERIVED), what
        for k in a:
            assert bits(np.asarray(a[k], dtype=np.asarray(b[k]).dtype), b[k]), (what, k, a[k], b[k])


def strided(beta, likes):
    """both tables inside larger allocations of NaN: another ld_t, an offset, likes with ld_c = 3; the gaps must never be read"""
    T, Cn = beta.shape
    bb = np.full((2 * T + 1, Cn + 3), np.nan)
    bb[1:2 * T + 1:2, 2:Cn + 2] = beta
    ll = np.full((2 * T + 1, Cn + 2, 3), np.nan, likes.dtype)
    ll[1:2 * T + 1:2, 1:Cn + 1, 1] = likes
    return bb, (slice(1, 2 * T + 1, 2), slice(2, Cn + 2)), ll, (slice(1, 2 * T + 1, 2), slice(1, Cn + 1), 1)


def check_accuracy(ev, likes, j):
    """the four sums of series j within (T 2^-53 + 2^-52) of their values in extended precision: T roundings of the additions at
    most (the strands make far fewer), 2^-52 for exp and the squares"""
    T = ev["T"]
    start = np.cumsum([0] + [len(m) for m in ev["members"]])
    k = int(np.searchsorted(start, j, side="right")) - 1
    rb = ev["rung_beta"]
    df = rb[j - 1] - rb[j] if j > start[k] else 0.0
    dr = rb[j] - rb[j + 1] if j + 1 < start[k + 1] else 0.0
    l = np.take_along_axis(likes, host(ev["hold"]).astype(np.int64), 1)[:, j].astype(np.float64)
    for a, s1, s2 in ((df * (l - ev["mx"][j]), "sf", "sf2"), (-dr * (l - ev["mn"][j]), "sr", "sr2")):
        w = np.where(a <= -512.0, np.longdouble(0), np.exp(a.astype(np.longdouble)))
        for key, val in ((s1, np.sum(w)), (s2, np.sum(w * w))):
            assert val >= 1 and abs(np.longdouble(ev[key][j]) - val) <= (T * 2.0 ** -53 + 2.0 ** -52) * val, (key, j, ev[key][j], val)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("which", sorted(SETS))
def test_evidence_equals_the_restatement(engine, which, T, dtype):
    import torch
    beta, likes, ladder = make_case(T, which, dtype)
    want = V.evidence(beta, likes, ladder, stats=package_stats(engine))
    Cn = ladder.size
    if T >= 257 and Cn > 1:      # the terms span the table path down to the dropped ones, and the 1 + x branch where it is meant
        a = np.concatenate([(want["rung_beta"][j - 1] - want["rung_beta"][j]) * (np.take_along_axis(likes, want["hold"].astype(np.int64), 1)[:, j]
                                                                                .astype(np.float64) - want["mx"][j]) for j in range(1, Cn)])
        assert np.any((a > -512.0) & (a < -1.0)) and np.any(a == 0.0)
        # (the steps of 64 geometric rungs are too small to reach -512 on these likes; the ladders of five and three do)
        assert Cn != 10 or (np.any(a <= -512.0) and np.any((a < 0) & (a > -2.0 ** -54)))
    if CONSTANT[which] is not None:
        j = CONSTANT[which]
        assert want["mx"][j] == want["mn"][j] == -777.0 and want["sf"][j] == T == want["sr2"][j]
    got = D.ladder_evidence(beta, likes, ladder, engine=engine)
    same_evidence(got, want, "host")
    for j in sorted({0, Cn - 1, Cn // 2, min(1, Cn - 1)}):
        check_accuracy(got, likes, j)
    ids, members, hold, rb = D.ladder_holders(beta, ladder, engine=engine)
    assert bits(ids, want["ids"]) and np.array_equal(hold, want["hold"]) and hold.dtype == np.int32 and bits(rb, want["rung_beta"])
    dev = torch.device("cuda", 0)
    got = D.ladder_evidence(torch.from_numpy(beta).to(dev), torch.from_numpy(likes).to(dev), ladder, engine=engine)
    assert got["hold"].is_cuda
    same_evidence(got, want, "device")
    bb, bsl, ll, lsl = strided(beta, likes)
    tb, tl = torch.from_numpy(bb).to(dev), torch.from_numpy(ll).to(dev)
    vb, vl = tb[bsl], tl[lsl]
    assert vb.data_ptr() != tb.data_ptr() and vl.data_ptr() != tl.data_ptr() and (Cn == 1 or vl.stride(1) == 3)
    assert T == 1 or (vb.stride(0) == 2 * bb.shape[1] and vl.stride(0) == 2 * ll.shape[1] * 3)
    same_evidence(D.ladder_evidence(vb, vl, ladder, engine=engine), want, "strided device")
    same_evidence(D.ladder_evidence(bb[bsl], ll[lsl], ladder, engine=engine), want, "strided host")
    h = D.ladder_holders(vb, ladder, engine=engine)
    assert h[2].is_cuda and np.array_equal(host(h[2]), want["hold"]) and bits(h[3], want["rung_beta"])


# ---- invariance -------------------------------------------------------------------------------------------------------------------
def test_a_ladder_has_the_same_bits_alone_among_others_and_shuffled(engine):
    T, L = 300, 40
    beta, likes, ladder = make_case(T, "2, 5, 3 interleaved", np.float32)
    full = D.ladder_evidence(beta, likes, ladder, maxlag=L, engine=engine)
    start = np.cumsum([0] + [len(m) for m in full["members"]])
    for k in range(3):
        cols = np.flatnonzero(ladder == k)
        alone = D.ladder_evidence(np.ascontiguousarray(beta[:, cols]), np.ascontiguousarray(likes[:, cols]), ladder[cols], maxlag=L, engine=engine)
        assert np.array_equal(cols[alone["hold"]], full["hold"][:, start[k]:start[k + 1]])
        for key in ("rung_beta",) + V.SUMS:
            assert bits(alone[key], full[key][start[k]:start[k + 1]]), (k, key)
        for key in STATS + DERIVED:
            assert bits(alone["ladders"][0][key], full["ladders"][k][key]), (k, key)
    perm = np.random.RandomState(4).permutation(ladder.size)
    shuf = D.ladder_evidence(np.ascontiguousarray(beta[:, perm]), np.ascontiguousarray(likes[:, perm]), ladder[perm], maxlag=L, engine=engine)
    assert np.array_equal(perm[shuf["hold"]], full["hold"])
    for key in ("rung_beta",) + V.SUMS:
        assert bits(shuf[key], full[key]), key
    for k in range(3):
        for key in STATS + DERIVED:
            assert bits(shuf["ladders"][k][key], full["ladders"][k][key]), (k, key)
    again = D.ladder_evidence(beta, likes, ladder, maxlag=L, engine=engine)
    assert all(bits(again[key], full[key]) for key in V.SUMS)
    # hold is a selection of the gathered calls: the sums of the table gathered on the host
    want = D.chain_series_stats(np.take_along_axis(likes, full["hold"].astype(np.int64), 1), L, engine=engine)
    got = D.chain_series_stats(likes, L, engine=engine, sel=full["hold"])
    assert all(bits(got[k], want[k]) for k in D.FIELDS + ("p",)) and got["x0"].shape == (ladder.size, 1)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def raw_evidence(engine, beta, likes, ladder, K, R, ld_hold=None, no_hold=False):
    """bh_chain_ladder_evidence on contiguous host tables with prefilled outputs: (rc, message, outputs)"""
    T, Cn = beta.shape
    lad = np.ascontiguousarray(ladder, np.int32)
    hold = np.full((T, Cn), -7, np.int32)
    outs = [np.full(Cn, FILL) for _ in range(7)]
    rc = engine._L.bh_chain_ladder_evidence(engine._h, E.HOST, None, T, Cn, Cn, E._ptr(beta), likes.itemsize, Cn, 1, E._ptr(likes), E._ptr(lad),
                                            K, R, None if no_hold else E._ptr(hold), Cn if ld_hold is None else ld_hold,
                                            *[E._ptr(o) for o in outs])
    return rc, engine._L.bh_engine_last_error(engine._h).decode(), [hold] + outs


def raw_holders(engine, beta, ladder, K, R, ld_hold=None):
    T, Cn = beta.shape
    lad = np.ascontiguousarray(ladder, np.int32)
    hold, rb = np.full((T, Cn), -7, np.int32), np.full(Cn, FILL)
    rc = engine._L.bh_chain_ladder_holders(engine._h, E.HOST, None, T, Cn, Cn, E._ptr(beta), E._ptr(lad), K, R, E._ptr(hold),
                                           Cn if ld_hold is None else ld_hold, E._ptr(rb))
    return rc, engine._L.bh_engine_last_error(engine._h).decode(), [hold, rb]


def untouched(outs):
    return np.all(outs[0] == -7) and all(np.all(o == FILL) for o in outs[1:])


def test_refusals_leave_the_outputs_untouched(engine):
    import torch
    rs = np.random.RandomState(3)
    ladder = [0] * 4 + [1] * 4
    T = 9
    beta = LR.permuted_betas(rs, T, ladder)
    likes = -5.0 - rs.uniform(0, 500.0, size=beta.shape)
    hold = V.holders(beta, ladder)[2]
    rc, _, outs = raw_evidence(engine, beta, likes, ladder, 2, 4)
    assert rc == E.BH_OK and not np.any(outs[0] == -7) and not any(np.any(o == FILL) for o in outs[1:])
    rc, _, nohold = raw_evidence(engine, beta, likes, ladder, 2, 4, no_hold=True)          # the sums alone
    assert rc == E.BH_OK and np.all(nohold[0] == -7) and all(bits(a, b) for a, b in zip(nohold[1:], outs[1:]))
    rc, _, houts = raw_holders(engine, beta, ladder, 2, 4)
    assert rc == E.BH_OK and np.array_equal(houts[0], outs[0]) and bits(houts[1], outs[1])
    cases = []
    b = beta.copy()
    b[4, hold[4, 2]] = b[4, hold[4, 1]]
    cases.append(("a tie at one row", "tied betas", dict(beta=b)))
    b = beta.copy()
    b[T - 1, hold[T - 1, 6]] *= 0.99
    cases.append(("a rung's beta changed at the last row", "the betas of a ladder change within the rows", dict(beta=b)))
    for v in (np.nan, np.inf, -np.inf):
        b, l = beta.copy(), likes.copy()
        b[5, 6] = v
        l[T - 1, 7] = v
        cases.append(("beta %r" % v, "a beta is not finite", dict(beta=b)))
        cases.append(("like %r" % v, "a like is not finite", dict(likes=l)))
    cases += [("a wrong R", "R must be", dict(R=3)), ("R too large", "R must be", dict(R=5)), ("ld_hold < C", "leading dimensions", dict(ld_hold=7)),
              ("an unused id", "every id used", dict(ladder=[0] * 4 + [2] * 4, K=3)), ("K = 0", "leading dimensions", dict(K=0))]
    for what, msg, kw in cases:
        args = dict(dict(beta=beta, likes=likes, ladder=ladder, K=2, R=4), **kw)
        rc, err, outs = raw_evidence(engine, **args)
        assert rc == E.BH_EINVAL and msg in err and untouched(outs), (what, rc, err)
        if "likes" not in kw:
            args.pop("likes")
            rc, err, outs = raw_holders(engine, **args)
            assert rc == E.BH_EINVAL and msg in err and untouched(outs), (what, rc, err)
    many = LR.permuted_betas(rs, 3, [0] * 65)
    rc, err, outs = raw_evidence(engine, many, -np.ones_like(many), [0] * 65, 1, 65)
    assert rc == E.BH_EUNSUPPORTED and "BH_LADDER_MAXRUNGS" in err and untouched(outs)
    rc, err, outs = raw_holders(engine, many, [0] * 65, 1, 65)
    assert rc == E.BH_EUNSUPPORTED and untouched(outs)
    bad = np.zeros((T, 8), np.float16)
    rc, err, outs = raw_evidence(engine, beta, bad, ladder, 2, 4)
    assert rc == E.BH_EINVAL and "float32 or float64" in err and untouched(outs)
    # the same through the functions, on device tensors
    dev = torch.device("cuda", 0)
    tb, tl = torch.from_numpy(beta).to(dev), torch.from_numpy(likes).to(dev)
    tied = tb.clone()
    tied[4, int(hold[4, 2])] = tied[4, int(hold[4, 1])]
    with pytest.raises(E.EngineError, match="tied betas"):
        D.ladder_evidence(tied, tl, ladder, engine=engine)
    with pytest.raises(E.EngineError, match="tied betas"):
        D.ladder_holders(tied, ladder, engine=engine)
    moved = tb.clone()
    moved[T - 1, int(hold[T - 1, 6])] *= 0.99
    with pytest.raises(E.EngineError, match="change within the rows"):
        D.ladder_holders(moved, ladder, engine=engine)
    nanl = tl.clone()
    nanl[2, 3] = float("nan")
    with pytest.raises(E.EngineError, match="like is not finite"):
        D.ladder_evidence(tb, nanl, ladder, engine=engine)
    with pytest.raises(ValueError):
        D.ladder_evidence(tb, likes, ladder, engine=engine)          # a device beta wants device likes
    with pytest.raises(ValueError):
        D.ladder_evidence(beta, likes[:-1], ladder, engine=engine)


# ---- the analytic ladder ----------------------------------------------------------------------------------------------------------
def test_the_analytic_ladder_on_the_gpu(engine):
    """tests/test_evidence_ref.py's ladder through the engine: ss, ss_rev and ti2 within 4 of their own errors of -2 log 101"""
    import torch
    beta, likes, ladder = V.analytic_ladder(0)
    dev = torch.device("cuda", 0)
    ev = D.ladder_evidence(torch.from_numpy(beta).to(dev), torch.from_numpy(likes).to(dev), ladder, maxlag=64, engine=engine)
    d = ev["ladders"][0]
    assert list(d["betas"]) == list(V.ANALYTIC_BETAS) and d["complete"] and d["beta_min"] == 0.0
    for name, value, err, dist in V.within_errors(d):
        print("%-7s %.6f +- %.6f: %.2f errors from %.6f" % (name, value, err, dist, V.ANALYTIC_LOGZ))
        assert err > 0 and dist <= 4.0, (name, value, err, dist)
    same_evidence(ev, V.evidence(beta, likes, ladder, maxlag=64, stats=package_stats(engine)), "analytic")


# ---- tempered runs end to end -----------------------------------------------------------------------------------------------------
def tempered(tmp, **kw):
    """the tempered set-up of tests/test_gpu_chain_diag_ladders.py: two ladders of four temperatures on the golden chain targets"""
    from test_gpu_chains import SETUPS, make_targets
    g = golden("chain_golden.npz")
    su = SETUPS["exp"]
    init = dict(su["init"], iter_burnin=kw.pop("iter_burnin"), iter_main=kw.pop("iter_main"), maxmodels=kw.pop("maxmodels"), savepath=str(tmp))
    ladder = np.repeat(np.arange(2), 4)
    betas = np.tile(1.0 / np.geomspace(1.0, 20.0, 4), 2)
    return DeviceChains(make_targets(g), 8, init, su["priors"], seed=5, betas=betas, ladder=ladder, **kw), betas


@pytest.fixture(scope="module")
def tempered_run(tmp_path_factory):
    """... exchanges every 20 iterations, recorded on the device, a main phase of 400 iterations thinned to 100 rows"""
    return tempered(tmp_path_factory.mktemp("evidence"), iter_burnin=280, iter_main=400, maxmodels=100, swap_every=20, record="device")[0].run()


def same_site(got, want_ev, ks, offset=0):
    assert sorted(got) == ["ids", "ladders", "logz", "logz_spread", "members"]
    assert np.array_equal(got["ids"], np.asarray(want_ev["ids"])[ks]) and got["ids"].dtype == np.int64
    assert all(np.array_equal(m, offset + want_ev["members"][k]) for m, k in zip(got["members"], ks))
    for d, k in zip(got["ladders"], ks):
        for key in STATS + DERIVED:
            assert bits(d[key], want_ev["ladders"][k][key]), (k, key)
    ss = [want_ev["ladders"][k]["ss"] for k in ks]
    assert got["logz"] == float(np.mean(ss))
    assert (got["logz_spread"] == float(np.std(ss, ddof=1))) if len(ks) > 1 else np.isnan(got["logz_spread"])


def test_ladder_evidence_of_a_tempered_run(tempered_run):
    dev = tempered_run
    got = dev.ladder_evidence()
    d = dev.samples_dev("p2")
    T = int(d["likes"].shape[0])
    assert T == 100 and dev.nswaps > 0
    beta, likes = d["beta"].cpu().numpy(), d["likes"].cpu().numpy()
    want = D.ladder_evidence(beta, likes, dev.ladder, engine=dev.engine)
    assert np.any(np.diff(want["hold"], axis=0) != 0)            # the rungs moved between the chains inside the phase
    same_site(got, want, [0, 1])
    assert [list(m) for m in got["members"]] == [[0, 1, 2, 3], [4, 5, 6, 7]]
    for lad in got["ladders"]:
        run_betas = 1.0 / np.geomspace(1.0, 20.0, 4)
        assert bits(lad["betas"], np.sort(run_betas)[::-1]) and lad["beta_min"] == run_betas.min() and not lad["complete"]
        free = ~lad["ess_truncated"]
        assert np.all(lad["ess"][free] <= T)
        assert np.all(lad["log_ratio_rev"] >= lad["log_ratio"] - 6.0 * (lad["ss_err"] + lad["ss_rev_err"]))     # a sanity bracket
        assert np.all(np.isfinite(lad["log_ratio"])) and np.isfinite(lad["ti2"]) and lad["ti_err"] > 0
    assert np.isfinite(got["logz"]) and got["logz_spread"] >= 0
    p1 = dev.ladder_evidence("p1", maxlag=7)
    d1 = dev.samples_dev("p1")
    same_site(p1, D.ladder_evidence(d1["beta"].cpu().numpy(), d1["likes"].cpu().numpy(), dev.ladder, maxlag=7, engine=dev.engine), [0, 1])

    class TwoRanks:
        def is_initialized(self):
            return True

        def get_world_size(self):
            return 2
    saved = dev.dist
    dev.dist = TwoRanks()
    try:
        with pytest.raises(E.EngineError, match="across ranks"):
            dev.ladder_evidence()
    finally:
        dev.dist = saved


def test_ladder_evidence_of_many_sites():
    """2 sites x 2 ladders x 2 temperatures (the set-up of tests/test_gpu_chain_diag_ladders.py): one dict per site"""
    from test_gpu_sites_priors import SITE_INIT, SITE_PRIORS, full_site
    g = golden("chain_golden.npz")
    st = bh.SiteTargets([full_site(g, s, "phase_rf") for s in range(2)], names=["st0", "st1"], per_site_x="all", per_site_rf=True)
    inits = [dict(SITE_INIT[s], iter_burnin=80, iter_main=200, maxmodels=50) for s in range(2)]
    ladder = np.array([10, 10, 11, 11, 12, 12, 13, 13])
    betas = np.tile([1.0, 0.25], 4)
    dev = DeviceChains(st, 4, inits, SITE_PRIORS[:2], seed=77, search="fast", betas=betas, ladder=ladder, swap_every=10, record="device").run()
    got = dev.ladder_evidence()
    assert isinstance(got, list) and len(got) == 2
    d = dev.samples_dev("p2")
    want = D.ladder_evidence(d["beta"].cpu().numpy(), d["likes"].cpu().numpy(), ladder, engine=dev.engine)
    for s in range(2):
        same_site(got[s], want, [2 * s, 2 * s + 1])
        assert list(got[s]["ids"]) == [10 + 2 * s, 11 + 2 * s] and [list(m) for m in got[s]["members"]] == [[4 * s, 4 * s + 1], [4 * s + 2, 4 * s + 3]]
        assert all(list(lad["betas"]) == [1.0, 0.25] and lad["log_ratio"].shape == (1,) for lad in got[s]["ladders"])


def test_ladder_evidence_refuses_untempered_runs_and_host_records():
    from test_gpu_chains import SETUPS, make_targets
    g = golden("chain_golden.npz")
    su = SETUPS["exp"]
    init = dict(su["init"], iter_burnin=280, iter_main=60, maxmodels=15)
    plain = DeviceChains(make_targets(g), 4, init, su["priors"], seed=5, record="device")
    with pytest.raises(E.EngineError, match="untempered"):
        plain.ladder_evidence()
    ladder = np.repeat(np.arange(2), 2)
    betas = np.tile([1.0, 0.2], 2)
    rec = DeviceChains(make_targets(g), 4, init, su["priors"], seed=5, betas=betas, ladder=ladder, swap_every=20, record="host")
    with pytest.raises(E.EngineError, match="record='device'"):
        rec.ladder_evidence()


def test_an_adapting_run_has_evidence_in_its_main_phase_only(tmp_path):
    """ladder_adapt moves the betas in the burn-in: that phase is refused, the main phase holds them"""
    dc, betas = tempered(tmp_path, iter_burnin=120, iter_main=80, maxmodels=80, swap_every=2, record="device", ladder_adapt={"every": 2})
    dc.run()
    sw = dc.ladder_swaps()
    assert np.all(sw["adaptations"] >= 1)
    with pytest.raises(E.EngineError, match="change within the rows"):
        dc.ladder_evidence("p1")
    got = dc.ladder_evidence("p2")
    for k, lad in enumerate(got["ladders"]):
        assert bits(lad["betas"], sw["betas"][k]) and lad["log_ratio"].shape == (3,) and np.all(np.isfinite(lad["log_ratio"]))
