"""The argument rules of the chain-diagnostics entry points (csrc/chain_tables.h: bh_chain_table_span, bh_chain_sel_span,
bh_chain_ladder_span, bh_chain_model_table, bh_chain_ladder_groups), without a GPU: the rules are pure functions exported by the
library.  Each is held to a restatement in plain Python written from the headers (it shares no code with the library; Python's
integers are exact, the span rules' factors are chosen so that the library's long double products are exact as well).

The last test replays tests/golden/chain_diag_refusals_golden.npz (recorded from the entry points of the commit before these
rules; tests/test_gpu_chain_diag_refusals.py tells how) against the pure functions: every recorded row whose refusal is the text of
one of the rules must get that code and that text from the rule itself, and the rules that the entry point asks before it must
accept the row.  This file also holds what both files need of the table: its columns and how a row becomes a call."""
import ctypes as C
import itertools

import numpy as np
import pytest

from conftest import golden

BH_OK, BH_EINVAL, BH_EUNSUPPORTED = 0, -1, -4
MAXLAYERS, MAXDEPTHS, MAXRUNGS, MAXLAG, MAXCOLS = 32, 63, 64, 2048, 64

T_SPAN = "bad T, C or leading dimensions"
T_SEL = "the selection: K >= 1 series, ld_sel >= K"
T_LSPAN = "bad T, C, K or leading dimensions"
T_ML = "row width 2*ML must be 2..64 (ML <= BH_POSTERIOR_MAXLAYERS)"
T_D = "depths: 0..BH_DIAG_MAXDEPTHS"
T_DEP = "the depths must be finite and strictly ascending"
T_IDS = "ladder ids must be 0..K-1"
T_USED = "ladder ids must be 0..K-1, every id used"
T_RUNGS = "a ladder of more than BH_LADDER_MAXRUNGS chains"
T_R = "R must be the size of the largest ladder"
MODEL_TEXTS, GROUP_TEXTS = (T_ML, T_D, T_DEP), (T_IDS, T_USED, T_RUNGS, T_R)


class Refusal(C.Structure):  # bh_chain_refusal (csrc/chain_tables.h)
    _fields_ = [("code", C.c_int), ("text", C.c_char_p)]

    def pair(self):
        return self.code, (self.text.decode() if self.text else None)


@pytest.fixture(scope="module")
def lib():
    from bayhunter_amd import engine as E
    L = E.load_library()
    i32p, i64 = C.POINTER(C.c_int32), C.c_int64
    for name, args in (("bh_chain_table_span", [i64, C.c_int, i64, i64, i64]), ("bh_chain_sel_span", [i64, C.c_int, C.c_int, i64]),
                       ("bh_chain_ladder_span", [i64, i64, C.c_int, i64]), ("bh_chain_model_table", [C.c_int, C.c_int, C.c_void_p]),
                       ("bh_chain_ladder_groups", [C.c_int, i32p, C.c_int, C.POINTER(C.c_int), i32p, i32p, C.POINTER(C.c_int)])):
        getattr(L, name).restype = Refusal
        getattr(L, name).argtypes = args
    return L


# ---- the restatements ------------------------------------------------------------------------------------------------------------
OK = (BH_OK, None)


def restated_table_span(T, Cn, width, ld_t, ld_c):
    ok = T >= 1 and Cn >= 1 and ld_t >= 1 and ld_c >= width and (T - 1) * ld_t + (Cn - 1) * ld_c + width < 2 ** 60
    return OK if ok else (BH_EINVAL, T_SPAN)


def restated_sel_span(T, K, sel, ld_sel):
    ok = K >= 1 and sel and ld_sel >= K and (T - 1) * ld_sel + K < 2 ** 60
    return OK if ok else (BH_EINVAL, T_SEL)


def restated_ladder_span(T, ld_t, Cn, ld_c):
    return OK if T * ld_t + Cn * ld_c < 2 ** 40 else (BH_EINVAL, T_LSPAN)


def restated_model_table(ML, D, dep):
    if not 1 <= ML <= MAXLAYERS:
        return BH_EINVAL, T_ML
    if not 0 <= D <= MAXDEPTHS or (D > 0 and dep is None):
        return BH_EINVAL, T_D
    d = [float(v) for v in dep[:D]] if D else []
    if any(v != v or abs(v) == float("inf") for v in d) or any(not b > a for a, b in zip(d, d[1:])):
        return BH_EINVAL, T_DEP
    return OK


def restated_groups(lad, K, R):
    """(code, text), start, member, largest of the ladders of the chains 0..len(lad)-1"""
    if any(not 0 <= k < K for k in lad):
        return (BH_EINVAL, T_IDS), None, None, None
    size = [sum(1 for k in lad if k == j) for j in range(K)]
    if 0 in size:
        return (BH_EINVAL, T_USED), None, None, None
    if max(size) > MAXRUNGS:
        return (BH_EUNSUPPORTED, T_RUNGS), None, None, None
    if R is not None and R != max(size):
        return (BH_EINVAL, T_R), None, None, None
    return OK, [sum(size[:j]) for j in range(K + 1)], [c for j in range(K) for c, k in enumerate(lad) if k == j], max(size)


def groups(lib, lad, K, R):
    """bh_chain_ladder_groups of a ladder vector: ((code, text), start, member, largest)"""
    n = len(lad)
    a = (C.c_int32 * max(n, 1))(*lad)
    start, member, largest = (C.c_int32 * (K + 1))(*([-7] * (K + 1))), (C.c_int32 * max(n, 1))(*([-7] * max(n, 1))), C.c_int(-7)
    r = lib.bh_chain_ladder_groups(n, a, K, C.byref(C.c_int(R)) if R is not None else None, start, member, C.byref(largest)).pair()
    return (r, list(start), list(member)[:n], largest.value) if r == OK else (r, None, None, None)


# ---- the rules against the restatements ------------------------------------------------------------------------------------------
def test_ladder_groups_equal_the_restatement_on_every_small_vector(lib):
    from bayhunter_amd.diagnostics import _ladders
    seen = set()
    for n in range(1, 6):
        for lad in itertools.product(range(-1, 6), repeat=n):
            for K in range(1, 7):
                want = restated_groups(lad, K, None)
                assert groups(lib, lad, K, None) == want, (lad, K)
                seen.add(want[0][1])
                if want[0] == OK:
                    ids, inv, members, R = _ladders(lad)
                    assert list(ids) == list(range(K)) and list(inv) == list(lad) and R == want[3]
                    assert [list(m) for m in members] == [want[2][want[1][k]:want[1][k + 1]] for k in range(K)]
                    tries = (want[3], want[3] - 1, want[3] + 1)
                else:
                    tries = (1,)  # (an earlier refusal wins whatever R says)
                for R in tries:
                    want = restated_groups(lad, K, R)
                    assert groups(lib, lad, K, R) == want, (lad, K, R)
                    seen.add(want[0][1])
    assert seen == {None, T_IDS, T_USED, T_R}
    # the largest ladder the kernels take, and one chain more
    for n, code in ((MAXRUNGS, BH_OK), (MAXRUNGS + 1, BH_EUNSUPPORTED)):
        for R in (None, n, 1):
            want = restated_groups([0] * n, 1, R)
            assert groups(lib, [0] * n, 1, R) == want
            assert want[0][0] == (code if R in (None, n) or code != BH_OK else BH_EINVAL)
    assert groups(lib, [0] * 65 + [1], 2, None)[0] == (BH_EUNSUPPORTED, T_RUNGS)
    assert groups(lib, [0] * 64 + [1] * 64, 2, 64)[0] == OK


def test_span_rules_equal_the_restatement(lib):
    P = 2 ** 30
    tables = [(T, Cn, w, ld_t, ld_c) for T in (-1, 0, 1, 3) for Cn in (-1, 0, 1, 4) for w in (1, 5) for ld_t in (-1, 0, 1, 40)
              for ld_c in (w - 1, w, w + 3)]
    # spans of 2^60 - 1, 2^60, 2^60 + 1 through the rows' term, and through the chains' term
    tables += [(P + 1, 1, w, P - 1, w) for w in (P - 2, P - 1, P, P + 1)] + [(P + 1, 1, 1, P, 1), (P + 1, 1, 1, P, 0)]
    tables += [(1, 2 ** 20 + 1, w, 1, 2 ** 40 - 1) for w in (2 ** 20 - 2, 2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1)]
    tables += [(3, 2 ** 20 + 1, 2 ** 20 - 3, 1, 2 ** 40 - 1), (4, 2 ** 20 + 1, 2 ** 20 - 3, 1, 2 ** 40 - 1), (2 ** 62, 1, 1, 2 ** 62, 1)]
    got = set()
    for a in tables:
        want = restated_table_span(*a)
        assert lib.bh_chain_table_span(*a).pair() == want, a
        got.add((want[0], a[0] >= 1 and a[1] >= 1 and a[3] >= 1 and a[4] >= a[2]))
    assert got == {(BH_OK, True), (BH_EINVAL, True), (BH_EINVAL, False)}
    assert [restated_table_span(P + 1, 1, w, P - 1, w)[0] for w in (P - 1, P, P + 1)] == [BH_OK, BH_EINVAL, BH_EINVAL]

    sels = [(T, K, s, ld) for T in (1, 3) for K in (-1, 0, 1, 6) for s in (0, 1) for ld in (K - 1, K, K + 2)]
    sels += [(2 ** 31, K, 1, 2 ** 29) for K in (2 ** 29 - 2, 2 ** 29 - 1, 2 ** 29, 2 ** 29 + 1)] + [(2 ** 31 + 1, 1, 1, 2 ** 29)]
    for a in sels:
        assert lib.bh_chain_sel_span(*a).pair() == restated_sel_span(*a), a
    assert [restated_sel_span(2 ** 31, K, 1, 2 ** 29)[0] for K in (2 ** 29 - 1, 2 ** 29)] == [BH_OK, BH_EINVAL]
    assert restated_sel_span(2 ** 31 + 1, 1, 1, 2 ** 29) == (BH_EINVAL, T_SEL)   # 2^60 + 1

    M = 2 ** 20
    lads = [(M, M - 1, 0, 0), (M, M, 0, 0), (M + 1, M, 0, 0), (1, 1, 0, 0), (2 ** 40 - 1, 1, 0, 0), (2 ** 40, 1, 0, 0), (2 ** 50, 2 ** 50, 0, 0)]
    lads += [(M, M - 1, 2 ** 10, ld_c) for ld_c in (2 ** 10 - 1, 2 ** 10, 2 ** 10 + 1)] + [(M, M - 1, 2 ** 10 + 1, 2 ** 10 - 1)]
    for a in lads:
        assert lib.bh_chain_ladder_span(*a).pair() == restated_ladder_span(*a), a
    assert [restated_ladder_span(*a)[0] for a in lads[:3] + lads[7:10]] == [BH_OK, BH_EINVAL, BH_EINVAL, BH_OK, BH_EINVAL, BH_EINVAL]


def test_model_table_rule_equals_the_restatement(lib):
    nan, inf = float("nan"), float("inf")
    base = [0.5 * j for j in range(64)]
    deps = [None, base]
    for at in (0, 31, 62):
        for v in (nan, inf, -inf, "equal", "descending"):
            d = list(base)
            d[at] = v if not isinstance(v, str) else (d[at - 1] if at else d[1]) - (0.0 if v == "equal" else 0.25)
            if at == 0 and isinstance(v, str):   # the first position: equal to, or above, the second
                d[0] = d[1] + (0.0 if v == "equal" else 0.25)
            deps.append(d)
    seen = set()
    for ML, D, dep in itertools.product((0, 1, 32, 33), (-1, 0, 1, 2, 32, 63, 64), deps):
        arr = np.array(dep, dtype=np.float64) if dep is not None else None
        want = restated_model_table(ML, D, dep)
        got = lib.bh_chain_model_table(ML, D, arr.ctypes.data if arr is not None else None).pair()
        assert got == want, (ML, D, dep)
        seen.add(want[1])
    assert seen == {None, T_ML, T_D, T_DEP}
    assert restated_model_table(1, 63, deps[2 + 10]) == (BH_EINVAL, T_DEP) and restated_model_table(1, 62, deps[2 + 10]) == OK  # NaN last


# ---- the recorded refusals: the table's columns, and a row as a call -----------------------------------------------------------
ENTRIES = ("bh_chain_diag_series", "bh_chain_diag_models", "bh_chain_diag_medians", "bh_chain_diag_series_sel", "bh_chain_diag_models_sel",
           "bh_chain_diag_medians_sel", "bh_chain_ladder_index", "bh_chain_ladder_holders", "bh_chain_ladder_evidence",
           "bh_chain_rank_series", "bh_chain_rank_models", "bh_ladder_sweep_create")
INTS = ("entry", "memspace", "elem", "T", "C", "Q", "ML", "D", "L", "K", "R", "G", "q0", "nq", "ld_t", "ld_c", "ld_sel", "ld_aux", "ldx_t",
        "ldx_c", "ld_out_t", "ld_out_c")
# the table's `nonnull`, bit b: x the table (the likes of bh_chain_ladder_evidence), beta, out1 the first output (x0, lo, occupancy,
# rung_beta, the plan), out2 the others, sel, dep, lad the ladder / group vector, aux the optional rung / hold, z, zf, tail, zt, zoff
POINTERS = ("x", "beta", "out1", "out2", "sel", "dep", "lad", "aux", "z", "zf", "tail", "zt", "zoff")
LADW = 72  # columns of lad and zoff: a row whose vector is read has C <= LADW

_buf = (C.c_double * 8)()
PTR = C.addressof(_buf)  # a pointer that is not null; never read: every recorded call returns before the first HIP call


def table_rows(g):
    """the rows of the table as dicts: the integers, the pointers as 0 / 1, and the arrays the rules read on the host"""
    g = {k: v for k, v in g.items()}  # (an NpzFile reads an array anew at every access)
    for i in range(g["entry"].size):
        row = {k: int(g[k][i]) for k in INTS}
        row.update({k: int(g["nonnull"][i]) >> b & 1 for b, k in enumerate(POINTERS)})
        row.update(lad_v=np.ascontiguousarray(g["lad"][i]), dep_v=np.ascontiguousarray(g["dep"][i]), zoff_v=np.ascontiguousarray(g["zoff"][i]),
                   code=int(g["o_code"][i]), text=str(g["texts"][int(g["o_text"][i])]))
        yield i, row


def call_entry(lib, h, row):
    """The entry point row["entry"] of the library on engine h with the row's arguments; returns (code, last error)."""
    r = row
    p = lambda k: PTR if r[k] else None
    arr = lambda k, v: v.ctypes.data if r[k] else None
    name = ENTRIES[r["entry"]]
    head = [h, r["memspace"], None]
    table = [r["elem"], r["T"], r["C"]]
    sums = [p("out1")] + [p("out2")] * 6
    sel = [r["K"], p("sel"), r["ld_sel"]]
    ladder = [r["T"], r["C"], r["ld_t"], p("beta")]
    rank = [r["G"], arr("lad", r["lad_v"]), p("zt"), arr("zoff", r["zoff_v"]), p("z"), p("zf"), p("tail"), r["ld_out_t"], r["ld_out_c"]]
    dep = arr("dep", r["dep_v"])
    a = {
        "bh_chain_diag_series": head + table + [r["Q"], r["ld_t"], r["ld_c"], p("x"), r["L"]] + sums,
        "bh_chain_diag_models": head + table + [r["ML"], r["ld_t"], r["ld_c"], p("x"), r["D"], dep, r["L"]] + sums,
        "bh_chain_diag_medians": head + table + [r["ld_t"], r["ld_c"], p("x"), p("out1"), p("out2")],
        "bh_chain_diag_series_sel": head + table + [r["Q"], r["ld_t"], r["ld_c"], p("x")] + sel + [r["L"]] + sums,
        "bh_chain_diag_models_sel": head + table + [r["ML"], r["ld_t"], r["ld_c"], p("x")] + sel + [r["D"], dep, r["L"]] + sums,
        "bh_chain_diag_medians_sel": head + table + [r["ld_t"], r["ld_c"], p("x")] + sel + [p("out1"), p("out2")],
        "bh_chain_ladder_index": head + ladder + [arr("lad", r["lad_v"]), r["K"], r["R"], p("sel"), r["ld_sel"], p("aux"), r["ld_aux"],
                                                   p("out1"), p("out2"), p("out2")],
        "bh_chain_ladder_holders": head + ladder + [arr("lad", r["lad_v"]), r["K"], r["R"], p("aux"), r["ld_aux"], p("out1")],
        "bh_chain_ladder_evidence": head + ladder + [r["elem"], r["ldx_t"], r["ldx_c"], p("x"), arr("lad", r["lad_v"]), r["K"], r["R"],
                                                      p("aux"), r["ld_aux"], p("out1")] + [p("out2")] * 6,
        "bh_chain_rank_series": head + table + [r["Q"], r["ld_t"], r["ld_c"], p("x")] + rank,
        "bh_chain_rank_models": head + table + [r["ML"], r["ld_t"], r["ld_c"], p("x"), r["D"], dep, r["q0"], r["nq"]] + rank,
    }.get(name)
    if name == "bh_ladder_sweep_create":
        plan = C.c_void_p()
        code = lib.bh_ladder_sweep_create(h, r["C"], arr("lad", r["lad_v"]), r["K"], C.byref(plan) if r["out1"] else None)
        assert not plan.value
    else:
        code = getattr(lib, name)(*a)
    return code, (lib.bh_engine_last_error(h) or b"").decode()


def test_the_rules_give_the_recorded_refusals(lib):
    """Every recorded row whose refusal carries the text of a rule gets that code and text from the rule; the rules asked before
    it accept the row."""
    span = lambda r, w: lib.bh_chain_table_span(r["T"], r["C"], w, r["ld_t"], r["ld_c"]).pair()
    selr = lambda r: lib.bh_chain_sel_span(r["T"], r["K"], r["sel"], r["ld_sel"]).pair()
    lspan = lambda r, ld, Cn=0, ld_c=0: lib.bh_chain_ladder_span(r["T"], ld, Cn, ld_c).pair()
    model = lambda r: lib.bh_chain_model_table(r["ML"], r["D"], r["dep_v"].ctypes.data if r["dep"] else None).pair()
    held = {t: 0 for t in (T_SPAN, T_SEL, T_LSPAN) + MODEL_TEXTS + GROUP_TEXTS}
    for i, r in table_rows(golden("chain_diag_refusals_golden.npz")):
        name, rec = ENTRIES[r["entry"]], (r["code"], r["text"])
        models, sel = "models" in name, name.endswith("_sel")
        width = 1 if "medians" in name else 2 * r["ML"] if models else r["Q"]
        if rec[1] in MODEL_TEXTS:
            assert models and model(r) == rec, (i, r)
        elif rec[1] == T_SPAN:
            assert span(r, width) == rec or ("medians" in name and r["T"] >= 2 ** 32), (i, r)
        elif rec[1] == T_SEL:
            assert sel and span(r, width) == OK and selr(r) == rec and (not models or model(r) == OK), (i, r)
        elif rec[1] == T_LSPAN:
            own = r["T"] < 1 or r["C"] < 1 or r["K"] < 1 or r["K"] > r["C"] or r["ld_t"] < r["C"]
            if name == "bh_chain_ladder_index":
                own = own or r["ld_sel"] < r["K"] or (r["aux"] and r["ld_aux"] < r["C"])
                spans = [lspan(r, r["ld_t"]), lspan(r, r["ld_sel"])] + ([lspan(r, r["ld_aux"])] if r["aux"] else [])
            else:
                evid = name == "bh_chain_ladder_evidence"
                own = own or (r["aux"] and r["ld_aux"] < r["C"]) or (evid and (r["ldx_t"] < 1 or r["ldx_c"] < 1))
                spans = [lspan(r, r["ld_t"])] + ([lspan(r, r["ld_aux"])] if r["aux"] else []) + (
                    [lspan(r, r["ldx_t"], r["C"], r["ldx_c"])] if evid else [])
            assert own or rec in spans, (i, r)
            if own:
                continue
        elif rec[1] in GROUP_TEXTS:
            lad = [int(v) for v in r["lad_v"][:r["C"]]]
            assert groups(lib, lad, r["K"], None if name == "bh_ladder_sweep_create" else r["R"])[0] == rec, (i, r)
            if name != "bh_ladder_sweep_create":
                assert lspan(r, r["ld_t"]) == OK
        else:
            continue
        held[rec[1]] += 1
    assert all(held.values()), held
