"""Every compiled build of the dispersion kernels, launched by the engine's own calls and checked against the oracle.

The library compiles 33 builds of the group kernel (swd_group_kernel.hip and the translation units that include it), 40 of the lane
kernel (swd_kernel.hip, bh_launch_swd) and 10 of the trial-per-lane kernel (swd_lean.hip).  Each is separately compiled machine code,
so each is run here: RECIPES maps every build to one engine configuration and call, and the launch record of that call
(bh_engine_last_swd_launches) must hold the build in the role it was meant for.  The results are held to the references of
tests/test_gpu_swd_fast.py and tests/test_gpu_swd_lean.py:
  * the reference's sequence (FASTM 0, the reference-sequence targets of FASTM 1, lane FAST 0, second roots): velocities and failure
    flags bit-identical to the oracle (bit-identical to surfdisp96, tests/test_oracle_swd.py);
  * the short refinement in the reference's arithmetic (FASTM 1 / 2, lane FAST 2, not FA): bit-identical to the oracle's
    restatement (search mode 2, scan mode 1), and evaluation for evaluation where the call carries the counters;
  * the fast arithmetic (FA builds, the trial-per-lane kernel): RTOL of the reference's sequence (achieved 2e-6), failure flags and
    the period from which a row is zero identical;
  * an instrumented build (PROF, CNTB, lean CNT) returns the bytes of the same call's plain build, and a call run twice returns
    the same bytes (the progress board, restarts in place and the pairing order are scheduling only).
The last test asserts that the builds launched are the compiled set less UNREACHABLE and that every launch feature was seen."""
import itertools
import os
import re

import numpy as np
import pytest

from conftest import REPO
from bayhunter_amd.synth import synth_models
from test_swd_group_plan import compiled_builds

RTOL = 1e-5       # north_star (tests/test_gpu_swd_fast.py, tests/test_gpu_swd_lean.py)
ACHIEVED = 2.0e-6
CSRC = os.path.join(REPO, "bayhunter_amd", "csrc")

# ---- the compiled set -------------------------------------------------------------------------------------------------------
# group: (FASTM, SIMPLE, PROF, ADAPT, CNTB, FA); lane: (IFUNC, LOOK, WPB, FAST, SIMPLE, FA) -- bh_launch_swd's BH_LANE_PICK_* ladder:
# wave type x trial lanes x wavefronts per workgroup x (FAST, SIMPLE, FA) in {(2,1,1), (2,1,0), (2,0,0), (0,1,0), (0,0,0)};
# lean: (J, CNT, 0, 0, 0, 0).
GROUP = {("group", tuple(int(x) for x in k)) for k in compiled_builds()}
LANE_SEQ = ((2, 1, 1), (2, 1, 0), (2, 0, 0), (0, 1, 0), (0, 0, 0))
LANE = {("lane", (i, l, w) + s) for i, l, w, s in itertools.product((1, 2), (0, 1), (1, 2), LANE_SEQ)}
LEAN = {("lean", (j, c, 0, 0, 0, 0)) for j, c in itertools.product((4, 8, 16, 32, 64), (0, 1))}
COMPILED = GROUP | LANE | LEAN
UNREACHABLE = {
    ("lane", (i, 0, w, 0, 1, 0)):
        "bh_launch_swd takes the SIMPLE build of the reference's sequence only with trial lanes (J > 1): one lane per model "
        "keeps the general build (the Love build's register count, measured faster there)"
    for i, w in itertools.product((1, 2), (1, 2))}

# ---- inputs ------------------------------------------------------------------------------------------------------------------
P60 = np.linspace(2.0, 60.0, 60)
P30 = np.linspace(2.0, 60.0, 30)
P1 = np.array([21.0])
PSETS = {"p60": P60, "p30": P30, "p1": P1}


def ragged_set(seed, B, L, nfull=6, nhalf=6, lvz=0.3, **kw):
    """B LVZ-rich ragged models in arrays of L layers, nfull of them at L layers and nhalf a half-space alone, shuffled"""
    rs = np.random.RandomState(seed)
    a = synth_models(rs, B - nfull - nhalf, L, lvz_frac=lvz, ragged=True, **kw)
    f = synth_models(rs, nfull, L, lvz_frac=lvz, ragged=False, **kw)
    s = synth_models(rs, nhalf, L, lvz_frac=0.0, ragged=True, **kw)
    nlay_s = np.ones(nhalf, dtype=np.int32)
    s[1][:, :] = 0.0
    out = [np.concatenate([a[0], f[0], nlay_s])] + [np.concatenate([a[i], f[i], s[i]], axis=1) for i in range(1, 5)]
    for i in range(1, 5):
        for b in range(B - nhalf, B):
            out[i][1:, b] = 0.0
    perm = rs.permutation(B)
    return [out[0][perm]] + [np.ascontiguousarray(x[:, perm]) for x in out[1:]]


INPUTS = {  # name: the models (h, vp, vs, rho layer-major [L, B]); the oracle's answers are computed on first use (Models)
    "mix": lambda: ragged_set(11, 331, 12),                     # several models per wavefront with forced lanes, else one
    "thin": lambda: ragged_set(733, 301, 4, nfull=4, nhalf=4, lvz=0.2),   # thin models to 60 s: the guard fires
    "deep": lambda: ragged_set(21, 2500, 21),                   # typical depth 12 in arrays of 21: two depth classes
    "look": lambda: ragged_set(31, 8257, 10),                   # 2065 wavefronts of 4 models x 16 trial lanes > 2048
    "big": lambda: ragged_set(41, 131137, 6),                   # 2050 wavefronts of one lane per model > 2048
    "gbig": lambda: ragged_set(51, 2200, 12),                   # 132 000 second roots > 2048 x 64: one lane each, WPB = 2
    "gmid": lambda: ragged_set(61, 1500, 12),                   # 90 000 second roots: one lane each, WPB = 1
}


class Models:
    """one input: the models and the oracle's answers, computed once per (target, search, scan)"""

    def __init__(self, oracle, name):
        self.O = oracle
        self.nlay, self.h, self.vp, self.vs, self.rho = INPUTS[name]()
        self.T = [np.ascontiguousarray(x.T) for x in (self.h, self.vp, self.vs, self.rho)]
        self.B = len(self.nlay)
        self.memo = {}

    def answer(self, tgt, search, scan=0):
        """oracle (vel, err, nevals, guarded) of target tgt = (iwave, igr, mode, flsph, pset); search 0 = the reference's
        sequence, 2 = the engine's guarded short refinement"""
        key = (tgt, search, scan)
        if key not in self.memo:
            iwave, igr, mode, flsph, pset = tgt
            self.O.set_swd_search(search)
            self.O.lib().bho_swd_set_scan(scan)
            self.O.swd_guarded_count(reset=True)
            try:
                v, e, n = self.O.swd_batch(self.nlay, *self.T, PSETS[pset], iwave, igr, mode=mode, flsph=flsph)
                g = self.O.swd_guarded_count(reset=True)
            finally:
                self.O.set_swd_search(0)
                self.O.lib().bho_swd_set_scan(0)
            self.memo[key] = (v, e, n, g)
        return self.memo[key]


# ---- recipes -----------------------------------------------------------------------------------------------------------------
R, L = 2, 1


def tg(iwave, igr=0, mode=1, flsph=0, pset="p60"):
    return (iwave, igr, mode, flsph, pset)


def rc(name, inp, targets, want, search="reference", arith="exact", G=0, look=0, trials=0, scan="steps", count=False, tun=None,
       feat=(), ev=False):
    """one engine configuration and call: its targets go through swd_batch (one) or evaluate_batch (two, or ev); want: the
    (family, role, key) launches the record must hold; feat: launch features it must show"""
    return dict(name=name, inp=inp, targets=tuple(targets), want=tuple(want), search=search, arith=arith, G=G, look=look,
                trials=trials, scan=scan, count=count, tun=dict(tun or {}), feat=tuple(feat), ev=ev or len(targets) > 1)


def gk(*k):
    return ("group", "main", tuple(int(x) for x in k))


def gr(*k):
    return ("group", "rerun", tuple(int(x) for x in k))


def lk(*k):
    return ("lane", "main", tuple(int(x) for x in k))


def ls(*k):
    return ("lane", "second", tuple(int(x) for x in k))


NR = {"swd_no_restart": 1}
NS = {"swd_no_simple": 1}
NL = {"swd_no_lean": 1}
RECIPES = [
    # group kernel, several models per wavefront (lanes forced: no ADAPT)
    rc("g2_R_prof", "mix", [tg(R)], [gk(2, 1, 1, 0, 0, 0)], "fast", G=9, look=2, count=True),
    rc("g2_L_prof_cntb", "mix", [tg(L)], [gk(2, 1, 1, 0, 1, 0)], "fast", G=9, look=2, count=True, scan="counted"),
    rc("g2_R", "mix", [tg(R, pset="p1")], [gk(2, 1, 0, 0, 0, 0)], "fast", G=9, look=2),
    rc("g2_L_cntb", "mix", [tg(L)], [gk(2, 1, 0, 0, 1, 0)], "fast", G=9, look=2, scan="auto"),
    rc("g2_R_nosimple", "mix", [tg(R)], [gk(2, 0, 1, 0, 0, 0)], "fast", G=9, look=2, tun=NS),
    rc("g2_L_nosimple_cntb", "mix", [tg(L)], [gk(2, 0, 1, 0, 1, 0)], "fast", G=9, look=2, tun=NS, scan="counted", count=True),
    rc("g1_RRg_mixed", "mix", [tg(R), tg(R, 1)], [gk(1, 0, 1, 0, 0, 0), gr(0, 0, 1, 0, 0, 0), ls(2, 1, 1, 0, 0, 0)], "fast", G=9,
       look=2, feat=("interleaved",)),
    rc("g1_RL_fast_rayleigh", "mix", [tg(R), tg(L)], [gk(1, 0, 1, 0, 0, 0), gr(0, 1, 0, 1, 0, 0)], "fast_rayleigh", G=9, look=2,
       feat=("interleaved",)),
    rc("g0_R_prof", "mix", [tg(R)], [gk(0, 1, 1, 0, 0, 0)], G=9, look=2, count=True),
    rc("g0_L_prof_cntb", "mix", [tg(L)], [gk(0, 1, 1, 0, 1, 0)], G=9, look=2, count=True, scan="counted"),
    rc("g0_R", "mix", [tg(R, pset="p1")], [gk(0, 1, 0, 0, 0, 0)], G=9, look=2),
    rc("g0_L", "mix", [tg(L, pset="p1")], [gk(0, 1, 0, 0, 1, 0)], G=9, look=2, scan="auto"),
    rc("g0_L_steps", "mix", [tg(L)], [gk(0, 1, 0, 0, 0, 0)], G=9, look=2, scan="steps"),
    rc("g0_Rg", "mix", [tg(R, 1)], [gk(0, 0, 1, 0, 0, 0), ls(2, 1, 1, 0, 0, 0)], G=9, look=2),
    rc("g0_Lm3_sph", "mix", [tg(L, 0, 3, 1, "p30")], [gk(0, 0, 1, 0, 1, 0)], G=9, look=2, scan="counted", count=True),
    rc("g0_Rm2_sph", "mix", [tg(R, 0, 2, 1, "p30")], [gk(0, 0, 1, 0, 0, 0)], G=9, look=2, count=True),
    # the fast arithmetic, several models per wavefront
    rc("gFA_R_prof", "mix", [tg(R)], [gk(2, 1, 1, 0, 0, 1)], "fast", "fast", G=9, look=2, count=True),
    rc("gFA_L_prof_cntb", "mix", [tg(L)], [gk(2, 1, 1, 0, 1, 1)], "fast", "fast", G=9, look=2, count=True, scan="counted"),
    rc("gFA_R", "mix", [tg(R, pset="p1")], [gk(2, 1, 0, 0, 0, 1)], "fast", "fast", G=9, look=2),
    rc("gFA_L_cntb_sph", "mix", [tg(L, flsph=1)], [gk(2, 1, 0, 0, 1, 1)], "fast", "fast", G=9, look=2, scan="auto"),
    # one model per wavefront (ADAPT; the planner's own choice for a few hundred models): restart in place, or the re-run launch
    rc("gA2_R_prof", "mix", [tg(R)], [gk(2, 1, 1, 1, 0, 0), gr(0, 1, 1, 1, 0, 0)], "fast", count=True, tun=NR),
    rc("gA2_L_prof_cntb", "thin", [tg(L, pset="p30")], [gk(2, 1, 1, 1, 1, 0), gr(0, 1, 1, 1, 1, 0)], "fast", count=True,
       scan="counted", tun=NR),
    rc("gA2_R", "mix", [tg(R, pset="p1")], [gk(2, 1, 0, 1, 0, 0), gr(0, 1, 0, 1, 0, 0)], "fast", tun=NR),
    rc("gA2_L_cntb", "thin", [tg(L, pset="p30")], [gk(2, 1, 0, 1, 1, 0), gr(0, 1, 0, 1, 1, 0)], "fast", scan="counted",
       tun=NR),
    rc("gA2_L_rerun_passes", "thin", [tg(L, pset="p30")], [gk(2, 1, 0, 1, 0, 0), gr(0, 1, 0, 1, 0, 0)], "fast",
       tun=dict(NR, swd_rerun_wgs=1), feat=("rerun_passes",)),
    rc("gA1_R_prof", "mix", [tg(R)], [gk(1, 1, 1, 1, 0, 0)], "fast", count=True, feat=("restart",)),
    rc("gA1_R", "thin", [tg(R, pset="p30")], [gk(1, 1, 0, 1, 0, 0)], "fast", feat=("restart",)),
    rc("gA1_L_cntb", "thin", [tg(L, pset="p30")], [gk(1, 1, 0, 1, 1, 0)], "fast", scan="counted", feat=("restart",)),
    rc("gA1_L_big", "thin", [tg(L, pset="p30")], [gk(1, 1, 1, 1, 1, 0)], "fast", scan="counted", count=True, feat=("restart",)),
    rc("gA0_R_prof", "mix", [tg(R)], [gk(0, 1, 1, 1, 0, 0)], count=True),
    rc("gA0_L_prof_cntb", "mix", [tg(L)], [gk(0, 1, 1, 1, 1, 0)], count=True, scan="counted"),
    rc("gA0_R", "mix", [tg(R, pset="p1")], [gk(0, 1, 0, 1, 0, 0)]),
    rc("gA0_L_cntb", "mix", [tg(L, flsph=1)], [gk(0, 1, 0, 1, 1, 0)], scan="counted"),
    rc("gAFA_R_prof", "mix", [tg(R)], [gk(2, 1, 1, 1, 0, 1), gr(0, 1, 1, 1, 0, 0)], "fast", "fast", count=True, tun=NL),
    rc("gAFA_L_prof_cntb", "thin", [tg(L, pset="p30")], [gk(2, 1, 1, 1, 1, 1), gr(0, 1, 1, 1, 1, 0)], "fast", "fast", count=True,
       scan="counted", tun=NL),
    rc("gAFA_R", "mix", [tg(R, pset="p1")], [gk(2, 1, 0, 1, 0, 1)], "fast", "fast", tun=NL),
    rc("gAFA_L_cntb", "thin", [tg(L, pset="p30")], [gk(2, 1, 0, 1, 1, 1), gr(0, 1, 0, 1, 1, 0)], "fast", "fast", scan="counted",
       tun=NL),
    # launch features: two depth classes, the SIMD-pairing order
    rc("g0_R_two_classes", "deep", [tg(R, pset="p30")], [gk(0, 1, 0, 0, 0, 0)], feat=("two_classes",)),
    rc("g1_RLg_pair", "mix", [tg(R, pset="p30"), tg(L, 1, pset="p30")], [gk(1, 0, 1, 0, 0, 0), gr(0, 0, 1, 0, 0, 0)], "fast", G=9,
       look=2, tun={"swd_pair_minwaves": 1}, feat=("pair_order", "interleaved")),
    # lane kernel, one wavefront per workgroup (lanes per model forced to 1)
    *[rc("lane_%s_J%d_%s" % ("L" if iw == L else "R", J, s), "mix", [tg(iw, 0, m, 0, ps)],
         [lk(iw, J > 1, 1, *k)] + ([gr(0, 1, co, 1, iw == L and sc == "counted", 0)] if k[0] == 2 else []),
         se, ar, G=1, look=J, tun=tu, scan=sc, count=co)
      for iw in (R, L) for J in (1, 4)
      for s, k, se, ar, tu, m, ps, sc, co in (
          ("FA", (2, 1, 1), "fast", "fast", {}, 1, "p60", "steps", False),
          ("S2", (2, 1, 0), "fast", "exact", {}, 1, "p60", "counted", True),
          ("N2", (2, 0, 0), "fast", "fast", NS, 1, "p1", "steps", False),
          ("S0" if J > 1 else "N0", (0, J > 1, 0), "reference", "exact", {}, 1, "p60", "counted", True),
          ("N0m2", (0, 0, 0), "reference", "exact", NS if J > 1 else {}, 2, "p1", "steps", False))],
    # lane kernel, two wavefronts per workgroup: more than 2048 wavefronts in the call
    *[rc("lane2_%s_J%d_%s" % ("L" if iw == L else "R", J, s), "look" if J > 1 else "big", [tg(iw, 0, 1, 0, "p1")],
         [lk(iw, J > 1, 2, *k)], se, ar, G=1, look=J, tun=tu)
      for iw in (R, L) for J in (1, 16)
      for s, k, se, ar, tu in (
          ("FA", (2, 1, 1), "fast", "fast", {}),
          ("S2", (2, 1, 0), "fast", "exact", {}),
          ("N2", (2, 0, 0), "fast", "exact", NS),
          ("S0" if J > 1 else "N0", (0, J > 1, 0), "reference", "exact", {}),
          *([("N0", (0, 0, 0), "reference", "exact", NS)] if J > 1 else []))],
    # the second roots of split group velocities: one lane per search, both time-slice classes (WPB 1 and 2)
    rc("second_R_wpb2", "gbig", [tg(R, 1)], [ls(2, 0, 2, 0, 0, 0)], feat=("second_wpb2",)),
    rc("second_L_wpb2", "gbig", [tg(L, 1)], [ls(1, 0, 2, 0, 0, 0)], feat=("second_wpb2",)),
    rc("second_R_wpb1", "gmid", [tg(R, 1)], [ls(2, 0, 1, 0, 0, 0)], feat=("second_wpb1",)),
    rc("second_L_wpb1", "gmid", [tg(L, 1)], [ls(1, 0, 1, 0, 0, 0)], feat=("second_wpb1",)),
    rc("second_L_look", "mix", [tg(L, 1)], [ls(1, 1, 1, 0, 0, 0)], scan="counted"),
    # the trial-per-lane kernel: every trial count, with and without the counters
    *[rc("lean_J%d_%s" % (J, "cnt" if c else "plain"), "mix", [tg(R if J in (4, 16, 64) else L, flsph=int(J == 8))] if J != 32
         else [tg(R), tg(L)], [("lean", "main", (J, c, 0, 0, 0, 0))], "fast", "fast", trials=J, count=bool(c))
      for J in (4, 8, 16, 32, 64) for c in (0, 1)],
]
FEATURES = ("two_classes", "interleaved", "pair_order", "restart", "rerun_passes", "second_wpb1", "second_wpb2")
BY_NAME = {r["name"]: r for r in RECIPES}


def test_the_tables_are_the_compiled_set():
    """(no GPU) the lane and lean builds stated above are what bh_launch_swd / bh_launch_swd_lean instantiate, the group builds what
    the translation units list; every recipe's intended build is compiled and not UNREACHABLE; names are unique"""
    src = open(os.path.join(CSRC, "swd_kernel.hip")).read()
    body = src[src.index("void bh_launch_swd(const SwdKernelArgs"):src.index("#undef BH_LANE_LAUNCH")]
    seq = set()
    for args in re.findall(r"swd_kernel<IF, LK, WP, ([^>]*)>", body):
        v = [x.strip() for x in args.split(",")]
        if v[0] == "FS":
            continue
        seq.add((int(v[0]), int(v[1] == "true"), int(len(v) > 2 and v[2] == "true")))
    for args in re.findall(r"BH_LANE_LAUNCH\(IF, LK, WP, (\d), (true|false)\)", body):
        seq.add((int(args[0]), int(args[1] == "true"), 0))
    assert seq == set(LANE_SEQ)
    assert "if (two) BH_LANE_PICK_FS(IF, LK, 2); else BH_LANE_PICK_FS(IF, LK, 1)" in body
    assert "if (J > 1) BH_LANE_PICK_WP(IF, true); else BH_LANE_PICK_WP(IF, false)" in body
    lean = open(os.path.join(CSRC, "swd_lean.hip")).read()
    lean = lean[lean.index("int bh_launch_swd_lean("):]
    assert sorted(int(j) for j in re.findall(r"case (\d+): LEAN_LAUNCH", lean)) == [4, 8, 16, 32]
    assert "default: LEAN_LAUNCH(64)" in lean and "swd_lean_kernel<JJ, true>" in lean and "swd_lean_kernel<JJ, false>" in lean
    assert len(GROUP) == 33 and len(LANE) == 40 and len(LEAN) == 10 and len(COMPILED) == 83
    assert set(UNREACHABLE) <= COMPILED
    assert len(BY_NAME) == len(RECIPES)
    wanted = set()
    for r in RECIPES:
        for fam, role, key in r["want"]:
            assert (fam, key) in COMPILED and (fam, key) not in UNREACHABLE, (r["name"], fam, key)
            wanted.add((fam, key))
        assert set(r["feat"]) <= set(FEATURES)
    assert wanted == COMPILED - set(UNREACHABLE), sorted(COMPILED - set(UNREACHABLE) - wanted)
    for f in FEATURES:
        assert any(f in r["feat"] for r in RECIPES), f


# ---- running a recipe ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs(oracle):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Models(oracle, name)
        return cache[name]
    return get


SEEN = {"launches": set(), "features": set(), "ran": set()}


def configure(eng, r):
    """apply recipe r (run_recipe restores what it changes: restore)"""
    eng.set_swd_search(r["search"])
    eng.set_swd_arith(r["arith"])
    eng.set_swd_scan(r["scan"])
    eng.set_swd_trials(r["trials"])
    eng.set_swd_group(r["G"])
    eng.set_swd_lookahead(r["look"])
    eng.set_instrumentation(False, r["count"])
    for k, v in r["tun"].items():
        eng.set_tuning(k, v)


def restore(eng, undo):
    """the engine's settings and the experiment switches back to what they were before the recipe (set_tuning is process-wide)"""
    eng.set_swd_group(0)
    eng.set_swd_lookahead(0)
    eng.set_instrumentation(False, False)
    for u in undo:
        if u[0] == "search":
            eng.set_swd_search(u[1])
        elif u[0] == "arith":
            eng.set_swd_arith(u[1])
        elif u[0] == "scan":
            eng.set_swd_scan(u[1])
        elif u[0] == "trials":
            eng.set_swd_trials(u[1])
        else:
            eng.set_tuning(u[1], u[2])


def call(eng, m, r):
    """the recipe's call: (vel per target [B, K], combined failure flags [B], launch record, neval or None)"""
    from bayhunter_amd import engine as E
    if not r["ev"]:
        iwave, igr, mode, flsph, pset = r["targets"][0]
        v, e = eng.swd_batch(m.nlay, m.h, m.vp, m.vs, m.rho, PSETS[pset], iwave, igr, mode=mode, flsph=flsph)
        vel = [v]
    else:
        descs = []
        for iwave, igr, mode, flsph, pset in r["targets"]:
            per = PSETS[pset]
            descs.append(dict(kind=E.TARGET_SWD, law=0, n=per.size, x=per, yobs=3.4 + 0.01 * per, iwave=iwave, igr=igr, mode=mode,
                              flsph=flsph))
        eng.set_targets(descs)
        noise = np.tile([0.0, 0.05] * len(descs), (m.B, 1))
        _, _, e, ymod = eng.evaluate_batch(m.nlay, m.h, m.vp, m.vs, noise, rho=m.rho, want_ymod=True)
        vel, o = [], 0
        for d in descs:
            vel.append(ymod[:, o:o + d["n"]])
            o += d["n"]
    rec = eng.last_swd_launches()
    n = eng.last_neval() if r["count"] else None
    return vel, e, rec, n


def takes_fast(r, t):
    iwave, igr, mode = t[:3]
    return igr == 0 and mode <= 1 and (r["search"] == "fast" or (r["search"] == "fast_rayleigh" and iwave == R))


def worst_rel(v, ov, ok):
    return float(np.max(np.abs(v[ok] - ov[ok]) / np.abs(ov[ok]))) if ok.any() else 0.0


def check_results(r, m, vel, err, rec):
    """each target against its reference; returns the number of guarded models the oracle's restatement re-ran"""
    fa = uses_fa(rec)
    oerr = np.zeros(m.B, dtype=bool)
    for t in r["targets"]:
        oerr |= m.answer(t, 0)[1] != 0
    assert np.array_equal(err != 0, oerr), (r["name"], "failure flags")
    # (evaluate_batch: the rows of the models every target of which succeeded; swd_batch: every row, zero rows included)
    ok = ~oerr if r["ev"] else np.ones(m.B, dtype=bool)
    guarded = 0
    for t, v in zip(r["targets"], vel):
        rv, re_, _, _ = m.answer(t, 0)
        if not takes_fast(r, t):
            assert np.array_equal(v[ok], rv[ok]), (r["name"], t, "reference's sequence")
        elif fa:
            assert np.array_equal(v[ok] == 0, rv[ok] == 0), (r["name"], t, "zero rows")
            both = (v != 0) & (rv != 0) & ok[:, None]
            w = worst_rel(v, rv, both)
            assert w <= RTOL and w <= ACHIEVED, (r["name"], t, w)
        else:
            fv, fe, _, g = m.answer(t, 2, 1)
            assert np.array_equal(fe, re_), (r["name"], t)       # (the restatement's flags are the reference's)
            assert np.array_equal(v[ok], fv[ok]), (r["name"], t, "restatement")
            guarded += g
    return guarded


def uses_fa(rec):
    """the call's main launch computes in the fast arithmetic (an FA build or the trial-per-lane kernel)"""
    return any(x["family"] == "lean" or (x["family"] != "lean" and x["key"][5] == 1) for x in rec if x["role"] == "main")


def expected_neval(r, m, rec):
    """the oracle's evaluation count of a one-target phase-velocity call, where the engine's is the restatement's count
    (tests/test_gpu_swd_fast.py); None where it is not comparable"""
    if r["ev"] or not r["count"] or r["scan"] == "auto":
        return None
    t = r["targets"][0]
    iwave, igr = t[:2]
    if igr != 0 or uses_fa(rec):
        return None
    counted = 0
    if iwave == L and r["scan"] == "counted":
        counted = 1
        if any(x["family"] == "group" and x["key"][4] == 0 for x in rec):   # (a build without the counted scan)
            return None
    return m.answer(t, 2 if takes_fast(r, t) else 0, counted)[2]


def plain_twin(r):
    """the same call on the uninstrumented build: no counters, every scan step evaluated"""
    return dict(r, count=False, scan="steps", name=r["name"] + "/plain")


def run_recipe(eng, m, r):
    undo = [("search", eng.swd_search()), ("arith", eng.swd_arith()), ("scan", eng.swd_scan()), ("trials", eng.swd_trials())]
    undo += [("tun", k, eng.tuning(k)) for k in r["tun"]]
    try:
        configure(eng, r)
        g0 = eng.guard_stats()[1]
        vel, err, rec, n = call(eng, m, r)
        counts, g1 = eng.guard_stats()[:2]
        vel2, err2, rec2, _ = call(eng, m, r)
    finally:
        restore(eng, undo)
    return vel, err, rec, n, list(counts), g1 - g0, vel2, err2, rec2


@pytest.mark.gpu
@pytest.mark.parametrize("name", [r["name"] for r in RECIPES])
def test_build(engine, inputs, name):
    r = BY_NAME[name]
    m = inputs(r["inp"])
    vel, err, rec, n, counts, reruns, vel2, err2, rec2 = run_recipe(engine, m, r)
    # the record holds the intended builds in their roles
    got = {(x["family"], x["role"], x["key"]) for x in rec}
    for w in r["want"]:
        assert w in got, (name, w, rec)
    assert rec == rec2, name
    SEEN["launches"] |= {(x["family"], x["key"]) for x in rec}
    # results
    guarded = check_results(r, m, vel, err, rec)
    for a, b in zip(vel, vel2):
        assert a.tobytes() == b.tobytes(), (name, "repeat")
    assert err.tobytes() == err2.tobytes(), (name, "repeat")
    ne = expected_neval(r, m, rec)
    if ne is not None:
        assert n == ne, (name, n, ne)
    # instrumented build (PROF, CNTB, lean CNT) = the plain build's bytes
    keys = [x for x in rec if x["family"] == "group" and (x["key"][2] or x["key"][4])] + \
           [x for x in rec if x["family"] == "lean" and x["key"][1]]
    if r["count"] or r["scan"] != "steps" or keys:
        twin = plain_twin(r)
        pv, pe, prec, _, _, _, _, _, _ = run_recipe(engine, m, twin)
        for a, b in zip(vel, pv):
            assert a.tobytes() == b.tobytes(), (name, "instrumented != plain")
        assert err.tobytes() == pe.tobytes(), name
        SEEN["launches"] |= {(x["family"], x["key"]) for x in prec}
    # launch features
    feats = set()
    main = [x for x in rec if x["role"] == "main"]
    if any(x["two_classes"] for x in main):
        feats.add("two_classes")
    if any(x["interleaved"] for x in main if x["family"] == "group"):
        feats.add("interleaved")
    if any(x["pair_order"] for x in main):
        feats.add("pair_order")
    if any(x["restart"] for x in main):
        feats.add("restart")
        assert reruns == 0, name                                # in place: no re-run launch
    rerun = [x for x in rec if x["role"] == "rerun"]
    if any(x["grid_x"] == 1 for x in rerun) and guarded >= 3 and sum(counts) >= 3:
        feats.add("rerun_passes")
    second = [x for x in rec if x["role"] == "second"]
    if any(x["key"][2] == 1 and x["fair"] > 0 for x in second):
        feats.add("second_wpb1")
    if any(x["key"][2] == 2 and x["fair"] > 0 for x in second):
        feats.add("second_wpb2")
    if not r["ev"] and takes_fast(r, r["targets"][0]) and not uses_fa(rec):
        assert sum(counts) == guarded, (name, counts, guarded)    # the guard fired on the models the restatement's did
    for f in r["feat"]:
        assert f in feats, (name, f, rec)
    SEEN["features"] |= feats
    SEEN["ran"].add(name)


@pytest.mark.gpu
def test_coverage_every_build_and_feature_ran():
    """runs last (file order): the builds launched are the compiled set less UNREACHABLE; every launch feature was seen"""
    assert SEEN["ran"] == set(BY_NAME), sorted(set(BY_NAME) - SEEN["ran"])
    reachable = COMPILED - set(UNREACHABLE)
    assert SEEN["launches"] == reachable, (sorted(reachable - SEEN["launches"]), sorted(SEEN["launches"] - reachable))
    assert SEEN["features"] == set(FEATURES), sorted(set(FEATURES) - SEEN["features"])
    print("\n%d of %d compiled dispersion builds launched; unreachable: %s" % (len(SEEN["launches"]), len(COMPILED),
                                                                             sorted(UNREACHABLE)))
