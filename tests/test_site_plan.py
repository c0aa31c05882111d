"""The site part of a fused call's plan (bh_plan_sites, csrc/engine_eval.hip), which needs no GPU, against the truth table of
tests/golden/site_plan_golden.npz: what the commit before the site half of plan_eval became this function decided, row by row.

The table was recorded once from that commit through a temporary export that was never committed.  It filled a
default-constructed bh_engine (no HIP call) from a row, called plan_eval, then eval_args_ok with non-null arguments, and returned
the plan's like, gauss[], x_table, rf_table, missing, rf_axis, laws, the first refusal's code and message text, and the two
expressions the launches evaluated on engine flags: `sitex && site_x_all` of launch_second_roots and `!site_x` under a class or
law launcher of run_like.  The rows are the reachable states: call {batch, sites} x the seven levels (sites from the shared table
up) x rf table x axis table (only with rf and a count table) x law table (only from missing_gauss up) x no_mfma x the target
lists {SWD nocorr}, {SWD, RF exp}, {SWD, RF gauss}, {RF gauss, RF gauss}, {SWD scaled, USER}, {RF gauss, USER} -- the last one
so that the refusal for a target without forward model competes with every other one -- x per target lacks (from missing up; a
Gauss-law target from missing_gauss up), own counts (RF, axes), another law (under a law table: both values on a Gauss-law
target, true elsewhere) and a class table (a Gauss-law target, any table).

Every field and the message text are equal on every row; the table reaches each of the seven refusals and each of the six
likelihood launchers."""
import ctypes as C

import numpy as np

from conftest import golden

LIKES = ("LIKE_PLAIN", "LIKE_SITES", "LIKE_SITES_X", "LIKE_SITES_M", "LIKE_SITES_C", "LIKE_SITES_L")


class Target(C.Structure):  # SitePlanAsk::Target (bh_device.h)
    _fields_ = [("kind", C.c_int), ("law", C.c_int), ("lacks", C.c_bool), ("rf_own_counts", C.c_bool), ("law_other", C.c_bool),
                ("classes", C.c_bool)]


class Ask(C.Structure):  # SitePlanAsk
    _fields_ = [("sites", C.c_bool), ("level", C.c_int), ("rf", C.c_bool), ("rf_axis", C.c_bool), ("laws", C.c_bool),
                ("no_mfma", C.c_bool), ("nt", C.c_int), ("t", Target * 8)]


class Plan(C.Structure):  # SitePlan
    _fields_ = [("x_table", C.c_bool), ("rf_table", C.c_bool), ("x_all", C.c_bool), ("missing", C.c_bool), ("rf_axis", C.c_bool),
                ("laws", C.c_bool), ("like", C.c_int), ("gauss", C.c_int * 8), ("desc_counts", C.c_bool), ("refusal", C.c_int),
                ("code", C.c_int)]


def library():
    from bayhunter_amd import engine as E
    lib = C.CDLL(E.LIB_PATH)
    plan = lib._Z13bh_plan_sitesRK11SitePlanAsk
    plan.restype, plan.argtypes = Plan, [C.POINTER(Ask)]
    text = lib._Z20bh_site_refusal_texti
    text.restype, text.argtypes = C.c_char_p, [C.c_int]
    return plan, text


def test_plan_sites_equals_the_recorded_truth_table():
    plan, text = library()
    g = {k: v for k, v in golden("site_plan_golden.npz").items()}
    texts = [str(s) for s in g["texts"]]
    n = g["nt"].size
    assert n > 7000
    user_beside_rf = 0
    refusals, likes = {}, set()
    for i in range(n):
        q = Ask(sites=bool(g["sites"][i]), level=int(g["level"][i]), rf=bool(g["rf"][i]), rf_axis=bool(g["axis"][i]),
                laws=bool(g["laws"][i]), no_mfma=bool(g["no_mfma"][i]), nt=int(g["nt"][i]))
        for t in range(q.nt):
            q.t[t] = Target(int(g["kind"][i, t]), int(g["law"][i, t]), bool(g["lacks"][i, t]), bool(g["own"][i, t]),
                            bool(g["other"][i, t]), bool(g["nclass"][i, t]))
        p = plan(C.byref(q))
        got = (p.like, list(p.gauss)[:q.nt], p.x_table, p.rf_table, p.missing, p.rf_axis, p.laws, p.code, text(p.refusal).decode())
        want = (int(g["o_like"][i]), [int(v) for v in g["o_gauss"][i, :q.nt]], bool(g["o_x_table"][i]), bool(g["o_rf_table"][i]),
                bool(g["o_missing"][i]), bool(g["o_rf_axis"][i]), bool(g["o_laws"][i]), int(g["o_code"][i]), texts[g["o_msg"][i]])
        assert got == want, "row %d: %r" % (i, {k: g[k][i].tolist() for k in g if not k.startswith("o_") and k != "texts"})
        assert (p.refusal == 0) == (p.code == 0) == (want[-1] == "")
        # (the two facts the launches took from the engine's flags before: second roots at a site's periods, the class call's counts)
        assert (p.x_all, p.desc_counts) == (bool(g["o_x_all"][i]), bool(g["o_desc_counts"][i])), "row %d" % i
        user_beside_rf += int(p.refusal == 1 and 1 in g["kind"][i, :q.nt])
        refusals.setdefault(p.refusal, want[-1])
        likes.add(p.like)
    assert sorted(refusals) == list(range(8)), "the table misses a refusal: %r" % sorted(refusals)
    assert len(set(refusals.values())) == 8 and all(text(r).decode() == m for r, m in refusals.items())
    assert user_beside_rf > 500, "the refusal for a target without forward model does not compete with the others"
    assert likes == set(range(len(LIKES))), "the table misses a likelihood launcher: %r" % sorted(likes)
