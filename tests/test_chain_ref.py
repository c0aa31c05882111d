"""tests/chain_ref.py -- the plain restatement of one chain step that csrc/chain_kernel.hip is compared with -- pinned to the
reference itself, and the crafted populations of tests/test_gpu_chain_kernels.py checked from the reference alone (no GPU).

golden/chain_step_golden.npz (gen_chain_step_golden.py) holds 718 single calls of the reference's own `iterate` with injected
draws and a stand-in likelihood, and what its methods returned: proposals, validity, dvs2, the layered model, alpha, counters,
adapted widths.  chain_ref reproduces them bit for bit; alpha to 4 ulp (the reference takes numpy's log of A).
"""
import math

import numpy as np
import pytest

from conftest import golden
import chain_ref as R


def fixture_cases():
    g = golden("chain_step_golden.npz")
    names = [str(s) for s in g["scalar_names"]]
    for i in range(g["scalars"].shape[0]):
        s = dict(zip(names, g["scalars"][i]))
        nt, n, ML = int(s["nt"]), int(s["n"]), int(s["ML"])
        none = lambda v: None if math.isnan(v) else v
        pr = R.make_priors(nt, ML, layers=(int(s["layermin"]), int(s["layermax"])), vs=(s["vsmin"], s["vsmax"]), z=(s["zmin"], s["zmax"]),
                           thickmin=s["thickmin"], lvz=none(s["lvz"]), hvz=none(s["hvz"]), vpvs=(s["vpvsmin"], s["vpvsmax"]),
                           mantle=None if math.isnan(s["mantle_vs"]) else (s["mantle_vs"], s["mantle_vpvs"]),
                           acceptance=(s["acc_lo"], s["acc_hi"]), noise_lo=g["noise_lo"][i, :2 * nt], noise_hi=g["noise_hi"][i, :2 * nt],
                           iter_burnin=int(s["iter_burnin"]), iterations=int(s["iterations"]), absent=int(s["absent"]))
        st = dict(n=n, vs=g["vs"][i, :n], z=g["z"][i, :n], vpvs=s["vpvs"], noise=g["noise"][i, :2 * nt], like=s["like"],
                  misfits=np.zeros(nt + 1), propdist=g["propdist"][i], proposed=g["proposed"][i], accepted=g["accepted"][i], naccepted=0)
        yield i, g, pr, st, int(s["iiter"]), g["draws"][i], s["newlike"]


def ulps(a, b):
    return abs(a - b) / np.spacing(max(abs(a), abs(b)))


def test_reproduces_the_recorded_reference_steps():
    seen_rules, seen_moves, count = set(), set(), 0
    for i, g, pr, st, iiter, d6, newlike in fixture_cases():
        move, valid, evaluated, accepted, pn = [int(v) for v in g["flags"][i]]
        tree = R.window(st, pr, d6[None, :], iiter, 1)
        p = tree["nodes"][0]
        seen_rules.add(p["rule"])
        seen_moves.add(p["move"])
        what = (i, p["rule"], sorted(p["notes"]))
        if move < 0:                      # the reference raised: np.argmin over no nucleus
            assert p["rule"] == "death_last" and not evaluated, what
            continue
        assert p["move"] == move and p["valid"] == bool(valid) == bool(evaluated), what   # `iterate`'s choice and the three _valid*
        nt = pr["nt"]
        if move <= 3:                     # _get_modelproposal (sorted), whether valid or not; dvs2 of a birth / death
            if p["raw"] is not None and "equal_depths" not in p["notes"]:
                assert p["raw"][0].size == pn, what
                if pn <= g["pvs"].shape[1]:
                    assert np.array_equal(p["raw"][0], g["pvs"][i, :pn]) and np.array_equal(p["raw"][1], g["pz"][i, :pn]), what
            else:
                assert p["rule"] == "capacity" and pn == st["n"] + 1, what
            if move >= 2:
                assert p["dvs2"] == g["dvs2"][i], what
        elif move == 4 and valid:
            assert np.array_equal(p["noise"], g["pnoise"][i, :2 * nt]), what
        elif move == 5 and valid:
            assert p["vpvs"] == g["pvpvs"][i], what
        if valid:                         # Models.get_vp_vs_h as handed to evaluate
            assert np.array_equal(p["h"], g["ph"][i, :p["n"]]) and np.array_equal(p["vp"], g["pvp"][i, :p["n"]]), what
        s1, dec, _ = R.accept(st, tree, [newlike], np.zeros((1, nt + 1)), d6[None, :], iiter, 1)
        if valid:
            assert ulps(dec[0]["alpha"], g["alpha"][i]) <= 4 and dec[0]["accepted"] == bool(accepted), what
            count += 1
        assert np.array_equal(s1["proposed"], g["proposed_out"][i]) and np.array_equal(s1["accepted"], g["accepted_out"][i]), what
        assert np.array_equal(s1["propdist"], g["propdist_out"][i]), what                   # adjust_propdist, or none
    assert seen_rules == set(R.RULES) - {"bad_record"} and seen_moves == set(range(6)) and count > 400


def test_fixture_covers_adaptation_and_the_early_boundary():
    adapted, early, late = 0, set(), set()
    for i, g, pr, st, iiter, d6, newlike in fixture_cases():
        adapted += int(not np.array_equal(g["propdist_out"][i], g["propdist"][i]))
        if g["flags"][i, 0] >= 0:
            (early if iiter <= -988 else late).add(int(g["flags"][i, 0]))
        if iiter % 1000 != 0:
            assert np.array_equal(g["propdist_out"][i], g["propdist"][i])
    assert adapted > 20 and not early & {2, 3} and {2, 3} <= late      # -988: no birth / death yet; -987: the first with them
    assert any(iiter == -987 and g["flags"][i, 0] in (2, 3) for i, g, _, _, iiter, _, _ in fixture_cases())


@pytest.mark.parametrize("kind,ML,nt,iiter", [("plain", 21, 3, R.LATE), ("priors", 4, 1, R.LATE), ("variant", 32, 8, R.crossing(3)),
                                              ("priors", 21, 3, 998)])
def test_window_is_the_sequential_walk(kind, ML, nt, iiter):
    """Every root-to-node path of the tree, for both outcomes of every decision, is `depth` single steps: the proposal at node j
    equals propose() from the state that accept() of single steps leaves when its decisions are forced along the path."""
    depth, C = 3, 37
    pop = R.population(kind, C, ML, nt, depth, iiter)
    tr = R.trees(pop)
    for c in range(C):
        pr, nodes = pop["priors"][c], tr[c]["nodes"]
        for leaf in range(3, 7):
            path = [leaf]
            while path[0] > 0:
                path.insert(0, (path[0] - 1) >> 1)
            st, reachable = pop["states"][c], True
            for k, j in enumerate(path):
                one = R.window(st, pr, pop["draws"][k:k + 1, :, c], iiter + k, 1)
                p, q = one["nodes"][0], nodes[j]
                assert q["reachable"] == reachable, (c, j)
                if reachable:
                    assert p["move"] == q["move"] and p["valid"] == q["valid"] and p["dvs2"] == q["dvs2"] and p["n"] == q["n"]
                    for f in ("vs", "z", "noise", "h", "vp", "rho"):
                        assert np.array_equal(p[f], q[f]), (c, j, f)
                if k + 1 < depth:
                    took = path[k + 1] == 2 * j + 2
                    # a single step with the decision forced: logL far above (accept) or far below (reject) the current one
                    st, dec, _ = R.accept(st, one, [st["like"] + (1e9 if took else -1e9)], np.zeros((1, nt + 1)),
                                          pop["draws"][k:k + 1, :, c], 1, 1)
                    if took and not p["valid"]:
                        reachable = False
                    else:
                        assert (len(dec) == 1 and dec[0]["accepted"] == took) or not p["valid"]


def hit(p, expect):
    return p["rule"] == expect[1] if expect[0] == "rule" else expect[1] in p["notes"]


@pytest.mark.parametrize("C,ML,nt,depth,wide", R.GPU_PARAMS)
def test_gpu_populations_hit_their_branches_and_keep_the_cap(C, ML, nt, depth, wide):
    """From the reference's own tags: every crafted chain hits the branch it was built for; the populations of the usual record
    hold the whole list; and at most 1 % of a population's chains (none of the designed ones) decide nearer to the threshold
    than the rounding budget of the double evaluation."""
    for build, pop in R.propose_populations(C, ML, nt, depth):
        tr = R.trees(pop)
        for c, label, expect in pop["designed"]:
            assert hit(tr[c]["nodes"][0], expect), (pop["kind"], pop["iiter"], c, label, tr[c]["nodes"][0]["rule"])
        labels = {l for _, l, _ in pop["designed"]}
        if pop["kind"] == "plain":
            assert labels == set(R.PROPOSE_BRANCHES)
        if pop["kind"] == "priors":
            assert sum(pop["priors"][c]["bad"] for c in range(C)) == 3
            assert all(not n["valid"] for c in range(C) if pop["priors"][c]["bad"] for n in tr[c]["nodes"])
            if pop["iiter"] == R.LATE:  # the birth with no room under the record whose capacity is below the shared one
                assert pop["designed"][0][1] == "birth_full" and pop["priors"][0]["layers"][1] + 1 < ML
                assert tr[0]["nodes"][0]["rule"] == "layers" and len(labels) >= 15
        notes = set().union(*[n["notes"] for t in tr for n in t["nodes"] if n["reachable"]])
        assert {"move_clamp", "move_first", "move_last"} <= notes      # (the chains whose draws sit on 0, 1 - 2^-53 and 1 at every level)
        if depth > 1 and pop["iiter"] < 0:                   # the window crosses the early-phase boundary
            assert "early" in tr[0]["nodes"][0]["notes"] or pop["priors"][0]["bad"]
            assert any("early" not in t["nodes"][-1]["notes"] for t in tr)
        assert any(not n["reachable"] for t in tr for n in t["nodes"]) == (depth > 1)
    for build, pop, beta in R.accept_populations(C, ML, nt, depth):
        tr = R.trees(pop)
        ap = R.accept_population(pop, tr, beta=beta)
        res = R.walk(pop, tr, ap)
        left = [c for c in range(C) if not R.counted(res[c][1])]
        assert len(left) <= C // 100, (pop["kind"], pop["iiter"], left)          # (no population has 100 chains: none is left out)
        notes = set().union(*[r[2] for r in res])
        if pop["iiter"] != R.LATE:
            assert set(R.ACCEPT_NOTES) <= notes, (pop["kind"], pop["iiter"], sorted(set(R.ACCEPT_NOTES) - notes))
        else:
            assert "adapt" not in notes
        if depth == 7:
            assert {"all_rejected_d7", "high_register"} <= notes
        by = dict((c, l) for c, l in ap["designed"])
        for c in range(C):
            dec, lab = res[c][1], by[c]
            if lab == "nan":
                assert dec == [] or not any(d["accepted"] for d in dec)
            if lab in ("just_above", "just_below") and tr[c]["nodes"][0]["valid"]:
                d = dec[0]
                assert d["accepted"] == (lab == "just_above") and (d["margin"] > 0) == d["accepted"]
                assert 1e-10 * abs(math.log(d["u"])) < abs(d["margin"]) < 1e-8 * abs(math.log(d["u"])), (c, d)
            if lab == "tie_u1":
                assert not any(d["accepted"] for d in dec)
            if lab in ("tie_u0", "all_accepted"):
                assert all(d["accepted"] for d in dec)
            for d in dec:                # the double decision is the exact one wherever it counts
                if not math.isnan(d["margin"]) and abs(d["margin"]) > d["budget"]:
                    assert d["accepted"] == (d["margin"] > 0)
