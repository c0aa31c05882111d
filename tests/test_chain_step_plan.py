"""The launch plan of the chain step (bh_plan_chain_step, csrc/chain_step.hip) and the twelve bh_chain_* entry points in front of it,
without a GPU: every refusal and every `C == 0` call returns before the first HIP call.

Part 1 -- refusals, against tests/golden/chain_step_plan_golden.npz: what the entry points of the commit before the planner returned,
row by row.  The table was recorded once from that commit's built library through its public entry points, by a throw-away script
that was never committed.  The script drew, per entry point, rows around one rule at a time (RULES below: the rule violated with
everything else in order -- several values of the violating field, several shapes -- and then the same violation with the other
fields drawn from small sets: C in {-1, 0, 1, 37}, depth in {0, 1, 2, 7, 8}, iiter in {-1001, -1000, -999, 0, 201, 998, 999, 1000},
nt in {-1, 0, 1, 8, 9}, maxlayers in {-1, 0, 4, 32, 33}, P in {0, 1, 4}, thinning in {0, 1, 7, 2^40}, pointers null or not, rows at
and one below row0 + m), plus rows with C == 0, in order and not, a few thousand per entry.  It issued a call only after checking
that the row has C == 0 or violates a rule that every copy of the rules refused (`never_launches` below is that check): no recorded
call could launch.  cfg, state and rec were real structures, the array pointers the address of a small host buffer.

The one intended difference: every entry point now refuses cfg->nt outside [0, BH_MAX_TARGETS] and cfg->maxlayers outside
[0, BH_CHAIN_MAXLAYERS].  The rows the parent accepted with such values (all at C == 0) must now give BH_EINVAL; they are counted
per entry, and the count must not be zero where the parent's copy of the rules lacked the check.

Part 2 -- positive plans against a restatement written here from the headers and DESIGN.md (it shares no code with the library):
kernel, grid, block, LDS bytes and the big-LDS flag of every entry at C in {1, 2, 37, 64, 65, 70}, depth 1..7, ld in {N C, N C + 3},
(maxlayers, nt) in {(4, 1), (21, 3), (32, 8)}; the record entries' due, due_step and m against a brute-force enumeration."""
import ctypes as C
import itertools

import pytest

from conftest import golden

BH_OK, BH_EINVAL = 0, -1
MAX_TARGETS, MAXLAYERS, MAXDEPTH = 8, 32, 7
ENTRIES = ("bh_chain_propose", "bh_chain_accept", "bh_chain_propose_window", "bh_chain_accept_window", "bh_chain_propose_sites",
           "bh_chain_propose_window_sites", "bh_chain_propose_priors", "bh_chain_propose_window_priors", "bh_chain_accept_priors",
           "bh_chain_accept_window_priors", "bh_chain_accept_window_record", "bh_chain_accept_window_priors_record")  # ChainEntry
ACCEPT = {e for e in ENTRIES if "accept" in e}
WINDOW = {e for e in ENTRIES if "window" in e}
SITES = {e for e in ENTRIES if e.endswith("_sites")}
TABLE = {e for e in ENTRIES if "priors" in e}
RECORD = {e for e in ENTRIES if e.endswith("_record")}
# the parent's copies of the rules that did not refuse every nt / maxlayers out of range (the record entries checked both bounds)
LACKED_RANGE = set(ENTRIES) - RECORD
KERNELS = ("none", "propose lane", "propose window", "accept lane", "accept wavefront")  # ChainKernel
REC_ARRAYS = ("rec_models", "rec_likes", "rec_vpvs", "rec_misfits", "rec_noise")
FIELDS = ("entry", "cfg", "state", "nt", "maxlayers", "C", "iiter", "depth", "ld", "logL", "misfits", "absent", "priors", "prior_of", "P",
          "rec") + REC_ARRAYS + ("rows", "thinning", "row0")
POINTERS = ("cfg", "state", "logL", "misfits", "absent", "priors", "prior_of", "rec") + REC_ARRAYS  # the table's `nonnull`: bit b


class Ask(C.Structure):  # ChainStepAsk (csrc/chain_step.h)
    _fields_ = [("entry", C.c_int), ("cfg", C.c_bool), ("state", C.c_bool), ("nt", C.c_int), ("maxlayers", C.c_int), ("C", C.c_int),
                ("iiter", C.c_int), ("depth", C.c_int), ("ld", C.c_int64), ("logL", C.c_bool), ("misfits", C.c_bool),
                ("absent", C.c_bool), ("priors", C.c_bool), ("prior_of", C.c_bool), ("P", C.c_int), ("rec", C.c_bool),
                ("rec_models", C.c_bool), ("rec_likes", C.c_bool), ("rec_vpvs", C.c_bool), ("rec_misfits", C.c_bool),
                ("rec_noise", C.c_bool), ("rows", C.c_int64), ("thinning", C.c_int64), ("row0", C.c_int64)]


BOOLS = {k for k, t in Ask._fields_ if t is C.c_bool}


class Plan(C.Structure):  # ChainStepPlan
    _fields_ = [("code", C.c_int), ("kernel", C.c_int), ("grid", C.c_uint), ("block", C.c_uint), ("lds", C.c_size_t),
                ("big_lds", C.c_bool), ("due", C.c_int), ("due_step", C.c_int), ("m", C.c_int)]


@pytest.fixture(scope="module")
def lib():
    from bayhunter_amd import engine as E
    L = E.load_library()
    L._Z18bh_plan_chain_stepRK12ChainStepAsk.restype = Plan
    L._Z18bh_plan_chain_stepRK12ChainStepAsk.argtypes = [C.POINTER(Ask)]
    return L


def plan(lib, row):
    """bh_plan_chain_step of a row (a dict over FIELDS); with a null cfg or store the ask holds zeros for what it would have read"""
    q = Ask(**{k: bool(row[k]) if k in BOOLS else int(row[k]) for k in FIELDS})
    if not row["cfg"]:
        q.nt = q.maxlayers = 0
    if not row["rec"]:
        for k in REC_ARRAYS:
            setattr(q, k, False)
        q.rows = q.thinning = q.row0 = 0
    return lib._Z18bh_plan_chain_stepRK12ChainStepAsk(C.byref(q))


_buf = (C.c_double * 8)()
PTR = C.addressof(_buf)  # a pointer that is not null; never read: every call of this file returns before a launch


def call_entry(lib, row):
    """The entry point `row["entry"]` of the library on the row's arguments."""
    from bayhunter_amd import engine as E
    name = ENTRIES[row["entry"]]
    ptr = lambda k: PTR if row[k] else None
    cfg, state, rec = E.ChainConfig(), E.ChainState(), E.ChainRecord()
    cfg.nt, cfg.maxlayers = int(row["nt"]), int(row["maxlayers"])
    for k in REC_ARRAYS:
        setattr(rec, k[4:], ptr(k))
    rec.rows, rec.thinning, rec.row0 = int(row["rows"]), int(row["thinning"]), int(row["row0"])
    a = [None, C.byref(cfg) if row["cfg"] else None, C.byref(state) if row["state"] else None, int(row["C"]), int(row["iiter"])]
    if name in WINDOW:
        a += [int(row["depth"]), int(row["ld"])]
    if name in ACCEPT:
        a += [ptr("logL"), ptr("misfits")]
    if name in SITES:
        a += [ptr("absent")]
    if name in TABLE:
        a += [ptr("priors"), int(row["P"]), ptr("prior_of")]
        if name not in ACCEPT:
            a += [ptr("absent")]
    if name in RECORD:
        a += [C.byref(rec) if row["rec"] else None]
    return getattr(lib, name)(*a)


def due_iterations(iiter, depth, thinning):
    return [i for i in range(iiter, iiter + depth) if i % thinning == 0]  # (Python's residue: non-negative)


RULES = ("C < 0", "depth", "ld", "adaptation inside the window", "cfg null", "state null", "logL null", "misfits null", "absent null",
         "priors null", "prior_of null", "P < 1", "rec null", "rec array null", "thinning < 1", "row0 < 0", "row0 + m > rows")
RANGE = "nt or maxlayers out of range"  # the rule only some of the parent's copies held


def applies(rule, name):
    return {"depth": name in WINDOW, "ld": name in WINDOW, "adaptation inside the window": name in WINDOW, "logL null": name in ACCEPT,
            "misfits null": name in ACCEPT, "absent null": name in SITES, "priors null": name in TABLE, "prior_of null": name in TABLE,
            "P < 1": name in TABLE, "rec null": name in RECORD, "rec array null": name in RECORD, "thinning < 1": name in RECORD,
            "row0 < 0": name in RECORD, "row0 + m > rows": name in RECORD}.get(rule, True)


def violations(row):
    """The rules a row violates, restated from the headers (a rule that cannot be evaluated -- it reads what another violated
    rule guards -- is not counted)."""
    name = ENTRIES[row["entry"]]
    v = set()
    depth, ld = (row["depth"], row["ld"]) if name in WINDOW else (1, row["C"])
    if row["C"] < 0:
        v.add("C < 0")
    if not row["cfg"]:
        v.add("cfg null")
    elif not (0 <= row["nt"] <= MAX_TARGETS and 0 <= row["maxlayers"] <= MAXLAYERS):
        v.add(RANGE)
    if not row["state"]:
        v.add("state null")
    if not 1 <= depth <= MAXDEPTH:
        v.add("depth")
    else:
        if ld < row["C"] * ((1 << depth) - 1):
            v.add("ld")
        if any((row["iiter"] + k) % 1000 == 0 for k in range(depth - 1)):
            v.add("adaptation inside the window")
    for k in ("logL", "misfits"):
        if name in ACCEPT and not row[k]:
            v.add(k + " null")
    if name in SITES and not row["absent"]:
        v.add("absent null")
    if name in TABLE:
        v |= {k + " null" for k in ("priors", "prior_of") if not row[k]}
        if row["P"] < 1:
            v.add("P < 1")
    if name in RECORD:
        if not row["rec"]:
            v.add("rec null")
        else:
            if not all(row[k] for k in REC_ARRAYS):
                v.add("rec array null")
            if row["thinning"] < 1:
                v.add("thinning < 1")
            if row["row0"] < 0:
                v.add("row0 < 0")
            if row["thinning"] >= 1 and 1 <= depth <= MAXDEPTH and row["row0"] + len(due_iterations(row["iiter"], depth, row["thinning"])) > row["rows"]:
                v.add("row0 + m > rows")
    return v


def never_launches(row):
    """C == 0, or a violation that every copy of the parent's rules refused: the condition under which the table was recorded"""
    return row["C"] == 0 or bool(violations(row) - {RANGE})


def test_refusals_equal_the_parent_commits_row_by_row(lib):
    g = {k: v for k, v in golden("chain_step_plan_golden.npz").items()}
    n = g["entry"].size
    assert 12 * 1500 < n < 12 * 5000
    codes = {e: set() for e in ENTRIES}
    alone = {e: set() for e in ENTRIES}
    newly = {e: 0 for e in ENTRIES}
    for i in range(n):
        row = {k: int(g[k][i]) for k in FIELDS if k not in POINTERS}
        row.update({k: int(g["nonnull"][i]) >> b & 1 for b, k in enumerate(POINTERS)})
        name, want = ENTRIES[row["entry"]], int(g["o_code"][i])
        v = violations(row)
        assert never_launches(row), "row %d could launch: %r" % (i, row)
        if RANGE not in v:
            assert want == (BH_EINVAL if v else BH_OK), "row %d: the restatement disagrees with the recorded code: %r" % (i, row)
        elif want == BH_OK:  # the parent's copy of the rules let it pass (at C == 0): the one intended difference
            assert v == {RANGE} and row["C"] == 0
            newly[name] += 1
            want = BH_EINVAL
        if len(v) == 1:
            alone[name] |= v
        codes[name].add(want)
        got = (call_entry(lib, row), plan(lib, row).code)
        assert got == (want, want), "row %d: %r, recorded %d: %r" % (i, got, want, row)
        assert plan(lib, row).kernel == 0
    for e in ENTRIES:
        assert codes[e] == {BH_OK, BH_EINVAL}, e
        missing = [r for r in RULES if applies(r, e) and r not in alone[e]]
        assert not missing, "%s: no row violates only %r" % (e, missing)
        assert (newly[e] > 0) if e in LACKED_RANGE else (newly[e] == 0), (e, newly[e])


# ---- part 2 ----------------------------------------------------------------------------------------------------------------------
def restated_plan(name, Cn, depth, ld, ML, nt):
    """(kernel, grid, block, LDS bytes, big) of a call in order, from the header comments and DESIGN.md: a lane per chain for one
    proposal in arrays of C columns and for the accept step of one iteration, a wavefront per chain for the accept walk of a window
    and for every call with a store; the window propose kernel with 2^(depth-1) lanes per chain in single-wavefront workgroups, the
    tree in LDS -- one record of 3 + 2 nt + 3 (ML + 1) doubles per node at an odd stride -- and, with a table of priors, the
    4 BH_MAX_TARGETS noise bounds of each of the workgroup's chains behind it; more than 64 KiB needs the allowance."""
    if name not in WINDOW:
        depth, ld = 1, Cn
    if name in ACCEPT:
        if name in RECORD or depth > 1:
            return "accept wavefront", Cn, 64, 0, False
        return "accept lane", -(-Cn // 64), 64, 0, False
    if depth == 1 and ld == Cn:
        return "propose lane", -(-Cn // 64), 64, 0, False
    chains = 64 // 2 ** (depth - 1)
    rec = 3 + 2 * nt + 3 * (ML + 1)
    rec += 1 - rec % 2
    doubles = chains * (2 ** depth - 1) * rec + (chains * 4 * MAX_TARGETS if name in TABLE else 0)
    return "propose window", -(-Cn // chains), 64, 8 * doubles, 8 * doubles > 64 * 1024


def in_order(name, Cn, depth, ld, ML, nt, iiter=1):
    row = dict.fromkeys(FIELDS, 1)
    row.update(entry=ENTRIES.index(name), nt=nt, maxlayers=ML, C=Cn, iiter=iiter, depth=depth, ld=ld, P=4, rows=1000, thinning=3, row0=5)
    return row


def test_plans_equal_the_restatement(lib):
    big = set()
    for name, Cn, depth, (ML, nt), pad in itertools.product(ENTRIES, (1, 2, 37, 64, 65, 70), range(1, 8), ((4, 1), (21, 3), (32, 8)), (0, 3)):
        ld = Cn * (2 ** depth - 1) + pad
        row = in_order(name, Cn, depth, ld, ML, nt)
        assert not violations(row)
        p = plan(lib, row)
        got = (p.code, KERNELS[p.kernel], p.grid, p.block, p.lds, p.big_lds)
        assert got == (BH_OK,) + restated_plan(name, Cn, depth, ld, ML, nt), (name, Cn, depth, ld, ML, nt)
        assert p.lds <= 160 * 1024
        if p.big_lds:
            big.add((name, ML, nt, depth))
    # the largest shape needs the allowance at depth 6 and 7, in every build of the window propose kernel
    for name in ("bh_chain_propose_window", "bh_chain_propose_window_sites", "bh_chain_propose_window_priors"):
        assert {(name, 32, 8, 6), (name, 32, 8, 7)} <= big
    assert all(name in WINDOW and name not in ACCEPT for name, _, _, _ in big)


def test_record_plans_equal_the_enumeration(lib):
    from bayhunter_amd.device_chains import snapshot_count
    seen = set()
    for name, thinning, iiter, depth in itertools.product(sorted(RECORD), (1, 2, 3, 7, 8, 1000, 2 ** 40), (-1007, -7, -6, 1, 993, 994),
                                                           range(1, 8)):
        due = due_iterations(iiter, depth, thinning)
        m = len(due)
        assert m == snapshot_count(iiter, iiter + depth, thinning)
        row = in_order(name, 37, depth, 37 * (2 ** depth - 1), 21, 3, iiter=iiter)
        row.update(thinning=thinning, rows=5 + m)
        assert not violations(row)
        p = plan(lib, row)
        assert (p.code, KERNELS[p.kernel], p.grid, p.m) == (BH_OK, "accept wavefront", 37, m), (name, thinning, iiter, depth)
        # the kernel takes a snapshot at level due, due + due_step, .. below depth
        assert [iiter + k for k in range(p.due, depth, p.due_step)] == due, (name, thinning, iiter, depth, p.due, p.due_step)
        assert p.due_step >= 1 and 0 <= p.due <= depth
        row["rows"] -= 1  # one row short of row0 + m
        assert plan(lib, row).code == BH_EINVAL
        seen.add(m)
    assert {0, 1, 2, 7} <= seen
