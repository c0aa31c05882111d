"""Plain numpy restatement of ONE rj-McMC chain step, written from the reference sampler (test infrastructure).

Sources: the reference's src/SingleChain.py -- the proposals (:246-328), the validity rules (:330-420), the width adaptation
and the acceptance probability (:425-487), `iterate` (:511-589) -- and src/Models.py:26-52 (nuclei -> layers, vp).  Nothing
here is taken from bayhunter_amd: the module imports nothing of the package and is what csrc/chain_kernel.hip is compared
with, decision by decision (tests/test_gpu_chain_kernels.py).  tests/test_chain_ref.py pins it to recorded outputs of the
reference's own methods (tests/golden/chain_step_golden.npz).

Conventions
  state   dict: n, vs[n], z[n], vpvs, noise[2nt], like, misfits[nt+1], propdist[5], proposed[5], accepted[5], naccepted
  priors  dict (make_priors): the reference's priors / initparams entries by name, plus what this project adds to a chain:
          `absent` (bit t: the chain's site lacks target t -- its two noise parameters are not free), `ML` (row capacity of
          the nuclei arrays, = layers max + 1 without a table of records) and `bad` (a record index out of range)
  draws   the six numbers one iteration consumes: u_move, u_index, u_z, u_accept, u_noise, normal; the reference's
          RandomState calls map to them as tests/philox_ref.InjectedRandomState does
A proposal is a few double-precision + - * / and comparisons in the order the reference fixes; numpy float64 does the same.
"""
import copy
import math

import mpmath
import numpy as np

MOVES = ("vsmod", "zvmod", "birth", "death", "noise", "vpvs")
PAR_MAP = {"vsmod": 0, "zvmod": 1, "birth": 2, "death": 2, "noise": 3, "vpvs": 4}
RULES = ("ok", "layers", "thickmin", "vs", "z", "lvz", "hvz", "noise", "vpvs", "capacity", "death_last", "bad_record")
TOP = 1.0 - 2.0 ** -53           # the largest double below 1


def make_priors(nt, ML, **kw):
    pr = dict(layers=(1, ML - 1), vs=(2.0, 5.0), z=(0.0, 60.0), thickmin=0.1, lvz=0.1, hvz=None, vpvs=(1.4, 2.1),
              mantle=(4.3, 1.8), acceptance=(40.0, 80.0), noise_lo=np.zeros(2 * nt), noise_hi=np.zeros(2 * nt),
              iter_burnin=1000, iterations=1300, absent=0, ML=ML, bad=False, nt=nt)
    pr.update(kw)
    pr["noise_lo"], pr["noise_hi"] = np.asarray(pr["noise_lo"], dtype=float), np.asarray(pr["noise_hi"], dtype=float)
    return pr


def noiseinds(pr):
    """the free noise parameters (SingleChain.py:146), less those of absent targets"""
    return np.array([i for i in range(2 * pr["nt"])
                     if pr["noise_lo"][i] != pr["noise_hi"][i] and not (pr["absent"] >> (i >> 1)) & 1], dtype=int)


def modifications(pr, iiter):
    """the list `iterate` chooses from (:512-517, :596-599)"""
    noisemods = ["noise"] if len(noiseinds(pr)) else []
    vpvsmods = ["vpvs"] if pr["vpvs"][0] != pr["vpvs"][1] else []
    if iiter < (-pr["iter_burnin"] + (pr["iterations"] * 0.01)):
        return ["vsmod", "zvmod"] + noisemods + vpvsmods
    return ["vsmod", "zvmod", "birth", "death"] + noisemods + vpvsmods


def _choice(seq, u, notes, what):
    k = int(u * len(seq))
    if k >= len(seq):
        notes.add(what + "_clamp")
        k = len(seq) - 1
    if k == len(seq) - 1:
        notes.add(what + "_last")
    if k == 0:
        notes.add(what + "_first")
    return seq[k]


def get_vp_vs_h(vs, z, vpvs, mantle, notes=None):
    """Models.py:26-52"""
    n = vs.size
    z_disc = (z[:n - 1] + z[1:n]) / 2.
    h = np.concatenate((z_disc - np.concatenate(([0], z_disc[:-1])), [0]))
    vp = vs * vpvs
    if mantle is not None:
        ind_m = np.where(vs >= mantle[0])[0]
        if len(ind_m):
            vp[ind_m[0]:] = vs[ind_m[0]:] * mantle[1]
            if notes is not None and np.any(vs[ind_m[0]:] < mantle[0]):
                notes.add("sticky_mantle")
    return vp, vs, h


def valid_model(vs, z, pr):
    """_validmodel (:330-392): the name of the first rule that fails, or 'ok'"""
    _, _, h = get_vp_vs_h(vs, z, 1.0, None)
    layermodel = h.size - 1
    if not (layermodel >= pr["layers"][0] and layermodel <= pr["layers"][1]):
        return "layers"
    if np.any(h[:-1] < pr["thickmin"]):
        return "thickmin"
    if np.any(vs < pr["vs"][0]) or np.any(vs > pr["vs"][1]):
        return "vs"
    zi = np.cumsum(h)
    if np.any(zi < pr["z"][0]) or np.any(zi > pr["z"][1]):
        return "z"
    if pr["lvz"] is not None:
        compvels = vs[1:] - (vs[:-1] * (1 - pr["lvz"]))
        if not compvels.size == compvels[compvels > 0].size:
            return "lvz"
    if pr["hvz"] is not None:
        compvels = (vs[:-1] * (1 + pr["hvz"])) - vs[1:]
        if not compvels.size == compvels[compvels > 0].size:
            return "hvz"
    return "ok"


def sort_model(vs, z, notes):
    """_sort_modelproposal (:315-328)"""
    if np.any(np.diff(z) == 0):
        notes.add("equal_depths")        # the reference's argsort is not stable there
    if np.all(np.diff(z) > 0):
        return vs, z
    ind = np.argsort(z, kind="stable")
    if np.max(np.abs(ind - np.arange(z.size))) >= 2:
        notes.add("jump")                # a nucleus passed two neighbours or more
    return vs[ind], z[ind]


def propose(state, pr, draws, iiter):
    """One proposal from `state` with the draws of iteration `iiter` -> dict: move (index into MOVES, -1 under a bad record),
    valid, rule, notes, n, vs, z, vpvs, noise, dvs2, h, vp, rho.  Invalid: the model parameters and layers are the base's.
    raw: the sorted model proposal (vs, z) before the validity rules, where one was formed (what _get_modelproposal returns)."""
    u_move, u_index, u_z, _, u_noise, normal = [np.float64(x) for x in draws]
    pd = np.asarray(state["propdist"], dtype=float)
    vs, z = np.array(state["vs"], dtype=float), np.array(state["z"], dtype=float)
    noise, vpvs = np.array(state["noise"], dtype=float), np.float64(state["vpvs"])
    n, notes, dvs2, rule, raw = vs.size, set(), np.float64(0.0), None, None

    def randint(high):                   # rstate.randint(0, high)
        k = int(u_index * high)
        if k >= high:
            notes.add("index_clamp")
        k = min(k, high - 1)
        notes.add("index_last" if k == high - 1 else "index_inner")
        return k

    if pr["bad"]:
        move, rule = -1, "bad_record"
    else:
        mods = modifications(pr, iiter)
        if len(mods) < 4 or "birth" not in mods:
            notes.add("early")
        modify = _choice(mods, u_move, notes, "move")
        move = MOVES.index(modify)
        if modify == "vsmod":
            ind = randint(n)
            vs[ind] = vs[ind] + (0.0 + pd[0] * normal)
        elif modify == "zvmod":
            ind = randint(n)
            z[ind] = z[ind] + (0.0 + pd[1] * normal)
        elif modify == "birth":
            z_birth = pr["z"][0] + u_z * (pr["z"][1] - pr["z"][0])
            dist = abs(z - z_birth)
            ind = np.argmin(dist)
            if np.sum(dist == dist[ind]) > 1:
                notes.add("nearest_tie")
            vs_before = vs[ind]
            vs_birth = vs_before + (0.0 + pd[2] * normal)
            dvs2 = np.square(vs_birth - vs_before)
            if n >= pr["ML"]:            # no row left: layers max + 1 nuclei already (the reference fails `layers`)
                rule = "capacity"
            else:
                z, vs = np.concatenate((z, [z_birth])), np.concatenate((vs, [vs_birth]))
        elif modify == "death":
            ind = randint(n)
            if n == 1:                   # the reference's argmin over nothing raises: no model with no nucleus
                rule = "death_last"
            else:
                z_before, vs_before = z[ind], vs[ind]
                z, vs = np.delete(z, ind), np.delete(vs, ind)
                dist = abs(z - z_before)
                near = np.argmin(dist)
                if np.sum(dist == dist[near]) > 1:
                    notes.add("nearest_tie")
                dvs2 = np.square(vs[near] - vs_before)
        elif modify == "noise":
            inds = noiseinds(pr)
            ind = _choice(inds, u_noise, notes, "noise")
            noise[ind] = noise[ind] + (0.0 + pd[3] * normal)
            rule = "ok"
            for idx in inds:
                if noise[idx] < pr["noise_lo"][idx] or noise[idx] > pr["noise_hi"][idx]:
                    rule = "noise"
                    if idx != ind and pr["noise_lo"][ind] <= noise[ind] <= pr["noise_hi"][ind]:
                        notes.add("noise_other")
        else:
            vpvs = vpvs + (0.0 + pd[4] * normal)
            rule = "vpvs" if (vpvs < pr["vpvs"][0] or vpvs > pr["vpvs"][1]) else "ok"
        if rule is None:
            vs, z = sort_model(vs, z, notes)
            raw = (vs.copy(), z.copy())
            rule = valid_model(vs, z, pr)
    valid = rule == "ok"
    if not valid:
        vs, z = np.array(state["vs"], dtype=float), np.array(state["z"], dtype=float)
        noise, vpvs = np.array(state["noise"], dtype=float), np.float64(state["vpvs"])
    vp, _, h = get_vp_vs_h(vs, z, vpvs, None if pr["bad"] else pr["mantle"], notes)
    return dict(move=move, valid=valid, rule=rule, notes=notes, n=vs.size, vs=vs, z=z, vpvs=vpvs, noise=noise, dvs2=dvs2,
                h=h, vp=vp, rho=vp * 0.32 + 0.77, raw=raw)


def applied(state, prop):
    """the state a valid proposal leads to once accepted (model parameters only; likelihood and counters: accept)"""
    s = dict(state)
    s.update(n=prop["n"], vs=prop["vs"].copy(), z=prop["z"].copy(), vpvs=prop["vpvs"], noise=prop["noise"].copy())
    return s


def window(state, pr, draws, iiter, depth):
    """The tree of a speculative window by its sequential definition: node j (heap order, children 2j+1 rejected / 2j+2
    accepted) is proposed from the state reached by walking root -> j and applying the proposal at every accepted edge.
    -> dict(nodes=[2^depth - 1 proposals, each with `reachable`], priors).  An accepted edge below an invalid node cannot
    be walked: what hangs below it is unreachable (proposed here from the unchanged state, contents of no interest)."""
    nodes = [None] * ((1 << depth) - 1)

    def build(j, k, base, reachable):
        p = propose(base, pr, draws[k], iiter + k)
        p["reachable"] = reachable
        nodes[j] = p
        if k + 1 < depth:
            build(2 * j + 1, k + 1, base, reachable)
            build(2 * j + 2, k + 1, applied(base, p) if p["valid"] else base, reachable and p["valid"])
    build(0, 0, state, True)
    return dict(nodes=nodes, priors=pr)


def adjust_propdist(propdist, proposed, accepted, acceptance, notes=None):
    """adjust_propdist (:425-450) -> the new widths"""
    propdist = np.array(propdist, dtype=float)
    with np.errstate(invalid="ignore", divide="ignore"):
        acceptrate = np.asarray(accepted, dtype=float) / np.asarray(proposed, dtype=float) * 100
    for i, rate in enumerate(acceptrate):
        if np.isnan(rate):
            continue
        if notes is not None and (rate == acceptance[0] or rate == acceptance[1]):
            notes.add("on_band")
        if rate < acceptance[0]:
            new = propdist[i] * 0.95
            if new < 0.001:
                new = 0.001
                if notes is not None:
                    notes.add("floor")
            propdist[i] = new
            if notes is not None:
                notes.add("below")
        elif rate > acceptance[1]:
            propdist[i] = propdist[i] * 1.05
            if notes is not None:
                notes.add("above")
        elif notes is not None:
            notes.add("inside")
    return propdist


def acceptance_probability(modify, like, cur, theta, dvs2, dv, beta=None):
    """get_acceptance_probability (:452-487) -> (alpha, A, B, dl); beta: the inverse temperature of a tempered chain
    (this project's addition: the likelihood difference enters as beta * (like - cur))"""
    dl = (like - cur) if beta is None else beta * (like - cur)
    if modify == "birth":
        A = (theta * np.sqrt(2 * np.pi)) / dv
        B = dvs2 / (2. * np.square(theta))
        return np.log(A) + B + dl, A, B, dl
    if modify == "death":
        A = dv / (theta * np.sqrt(2 * np.pi))
        B = dvs2 / (2. * np.square(theta))
        return np.log(A) - B + dl, A, -B, dl
    return dl, None, np.float64(0.0), dl


def margin(A, B, dl, u):
    """alpha - log(u) from the double operands at 60 digits, and the rounding budget of the double evaluation:
    64 * 2^-53 * (|log A| + |B| + |dl| + |log u|) -> (margin, budget) as floats (nan / +-inf where an operand is)"""
    if math.isnan(dl) or math.isnan(B):
        return float("nan"), 0.0
    if u == 0.0:
        return float("inf"), 0.0
    if math.isinf(dl):
        return float(dl), 0.0
    with mpmath.workdps(60):
        la = mpmath.log(mpmath.mpf(float(A))) if A is not None else mpmath.mpf(0)
        lu = mpmath.log(mpmath.mpf(float(u)))
        m = la + mpmath.mpf(float(B)) + mpmath.mpf(float(dl)) - lu
        budget = 64 * mpmath.mpf(2) ** -53 * (abs(la) + abs(float(B)) + abs(float(dl)) + abs(lu))
        return float(m), float(budget)


def accept(state, tree, logL, misfits, draws, iiter, depth, beta=None):
    """Walk the realised path through `tree` (logL [N], misfits [N][nt+1] per node): counters, naccepted, the width
    adaptation at (iiter + k) % 1000 == 0, commit of the last accepted node -> (new state, decisions, notes).
    decisions: one dict per valid proposal on the path -- k, node, move, alpha, u, accepted, margin, budget."""
    pr, nodes = tree["priors"], tree["nodes"]
    s = copy.deepcopy({k: v for k, v in state.items()})
    for k in ("propdist", "proposed", "accepted"):
        s[k] = np.array(s[k], dtype=float)
    dv = np.float64(pr["vs"][1]) - np.float64(pr["vs"][0])
    node, last, cur, decisions, notes = 0, -1, np.float64(s["like"]), [], set()
    for k in range(depth):
        p, accepted = nodes[node], False
        adapt_now = (iiter + k) % 1000 == 0
        if p["valid"]:
            modify = MOVES[p["move"]]
            paridx = PAR_MAP[modify]
            s["proposed"][paridx] += 1
            u = np.float64(draws[k][3])
            like = np.float64(logL[node])
            with np.errstate(all="ignore"):
                alpha, A, B, dl = acceptance_probability(modify, like, cur, s["propdist"][2], p["dvs2"], dv, beta)
                accepted = bool(np.log(u) < alpha)
            m, budget = margin(A, B, dl, u)
            decisions.append(dict(k=k, node=node, move=p["move"], alpha=alpha, u=u, accepted=accepted, margin=m, budget=budget))
            if accepted:
                last, cur = node, like
                s["accepted"][paridx] += 1
                s["naccepted"] += 1
            if adapt_now:
                if np.all(s["proposed"]) != 0:
                    notes.add("adapt")
                    s["propdist"] = adjust_propdist(s["propdist"], s["proposed"], s["accepted"], pr["acceptance"], notes)
                else:
                    notes.add("zero_proposed")
        elif adapt_now:
            notes.add("invalid_at_adapt")
        node = 2 * node + (2 if accepted else 1)
    if last >= 0:
        p = nodes[last]
        s.update(n=p["n"], vs=p["vs"].copy(), z=p["z"].copy(), vpvs=p["vpvs"], noise=p["noise"].copy(), like=cur,
                 misfits=np.array(misfits[last], dtype=float))
    else:
        notes.add("unchanged")
    if last >= 64:
        notes.add("high_register")
    if node == 2 * 63 + 1 and depth == 7:
        notes.add("all_rejected_d7")
    return s, decisions, notes


def counted(decisions):
    """True if every decision of a walk is further from its threshold than the rounding budget (NaN: a plain reject)"""
    return all(math.isnan(d["margin"]) or abs(d["margin"]) > d["budget"] or (d["margin"] == 0.0 and d["budget"] == 0.0)
               for d in decisions)       # (margin 0 with budget 0: log(1) against a difference of equal numbers, exact on both sides)


# ---------------------------------------------------------------------------------------------------------------------------
# Crafted populations.  Every crafted chain names the branch it is built to hit and how the reference shows that it did: a
# `rule` tag or a note of propose().  tests/test_chain_ref.py asserts those from this module alone.

def noise_bounds(nt):
    """free, fixed and (through `absent`) absent noise slots interleaved: sigma free everywhere, corr free at every third target"""
    lo, hi = np.zeros(2 * nt), np.zeros(2 * nt)
    for t in range(nt):
        lo[2 * t], hi[2 * t] = (0.2, 0.8) if t % 3 == 0 else (0.25 * (t % 2), 0.25 * (t % 2))
        lo[2 * t + 1], hi[2 * t + 1] = 1e-4, 0.05 + 0.01 * t
    return lo, hi


def records(nt, ML):
    """Four sets of priors that differ in every field.  0: the usual one.  1: zmin > 0, no mantle, no lvz, hvz, a dyadic thickmin,
    a smaller capacity (layers max + 1 < ML where ML allows).  2: fixed vp/vs, all sigmas fixed but one.  3: another band."""
    lo, hi = noise_bounds(nt)
    lo2, hi2 = lo.copy(), hi.copy()
    hi2[3::2] = lo2[3::2] = 0.02
    cap1 = max(1, (ML - 1) // 2)
    return [
        make_priors(nt, ML, noise_lo=lo, noise_hi=hi),
        make_priors(nt, ML, layers=(0, cap1), vs=(2.5, 4.5), z=(5.0, 50.0), thickmin=0.5, lvz=None, hvz=0.5, vpvs=(1.5, 2.0),
                    mantle=None, acceptance=(30.0, 60.0), noise_lo=lo * 0.5, noise_hi=hi * 2),
        make_priors(nt, ML, layers=(min(2, ML - 1), ML - 1), vs=(1.5, 4.8), z=(0.0, 80.0), thickmin=0.25, lvz=0.2, hvz=0.4,
                    vpvs=(1.73, 1.73), mantle=(4.2, 1.75), acceptance=(10.0, 20.0), noise_lo=lo2, noise_hi=hi2),
        make_priors(nt, ML, layers=(1, ML - 1), vs=(2.0, 5.5), z=(1.0, 70.0), thickmin=0.125, lvz=0.25, hvz=0.75, vpvs=(1.6, 1.9),
                    mantle=(4.0, 1.9), acceptance=(45.0, 55.0), noise_lo=lo, noise_hi=hi * 1.5),
    ]


def random_model(pr, n, rs):
    """n nuclei that pass every validity rule of pr"""
    zmin, zmax = pr["z"]
    vsmin, vsmax = pr["vs"]
    z = zmin + (zmax - zmin) * (np.arange(n) + 0.5 + 0.2 * rs.uniform(-1, 1, n)) / n
    vs = vsmin + (vsmax - vsmin) * (0.3 + 0.3 * (np.arange(n) + rs.uniform(0, 0.5, n)) / n)
    return vs, z


def random_state(pr, rs, n=None, wide=False):
    nt = pr["nt"]
    cap = min(pr["ML"], pr["layers"][1] + 1)
    if n is None:
        n = int(rs.randint(max(1, pr["layers"][0] + 1), cap + 1))
    vs, z = random_model(pr, n, rs)
    lo, hi = pr["noise_lo"], pr["noise_hi"]
    return dict(n=n, vs=vs, z=z, vpvs=pr["vpvs"][0] + rs.uniform(0.1, 0.9) * (pr["vpvs"][1] - pr["vpvs"][0]),
                noise=lo + rs.uniform(0.1, 0.9, 2 * nt) * (hi - lo), like=-100.0 + rs.normal(), misfits=rs.uniform(0, 1, nt + 1),
                propdist=np.array([0.3, 3.0, 0.3, 0.02, 0.1]) if wide else np.array([0.015, 0.015, 0.015, 0.005, 0.005]),
                proposed=np.zeros(5), accepted=np.zeros(5), naccepted=0)


def _u_for(modify, pr, iiter):
    mods = modifications(pr, iiter)
    return None if modify not in mods else (mods.index(modify) + 0.5) / len(mods)


def _exact_h(pr, vs3):
    """three nuclei with one layer exactly thickmin thick by the reference's own arithmetic, valid with vs3 -> (z, layer) or None"""
    t, zmin = pr["thickmin"], pr["z"][0]
    for z, k in ((np.array([zmin + 8.0, zmin + 8.0 + t, zmin + 8.0 + 2 * t]), 1), (np.array([zmin + 1.0, zmin + 1.0 + t, zmin + 1.0 + 2 * t]), 1),
                 (np.array([0.0, 2 * t, 2 * t + 8.0]), 0)):
        if get_vp_vs_h(vs3, z, 1.0, None)[2][k] == t and np.all(np.diff(z) > 0) and valid_model(vs3, z, pr) == "ok":
            return z, k
    return None


def crafted_propose(pr, iiter, rs):
    """-> list of (label, state, draws6, expect) for the root proposal under pr at iteration iiter.  expect: ('rule', tag),
    ('note', name) or ('valid', bool).  Cases that pr or the phase of iiter does not allow are left out."""
    out = []
    nt, cap = pr["nt"], min(pr["ML"], pr["layers"][1] + 1)
    nmin = max(1, pr["layers"][0] + 1)

    def add(label, st, expect, modify, **d):
        u = _u_for(modify, pr, iiter) if modify is not None else d.pop("u_move")
        if u is None:
            return
        dr = dict(u_move=u, u_index=rs.uniform(), u_z=rs.uniform(), u_accept=rs.uniform(), u_noise=rs.uniform(), normal=0.0)
        dr.update(d)
        out.append((label, st, np.array([dr[k] for k in ("u_move", "u_index", "u_z", "u_accept", "u_noise", "normal")]), expect))

    # birth with no room left: n == ML, or n == layers max + 1 < ML under a table of records
    add("birth_full", random_state(pr, rs, n=cap), ("rule", "capacity" if cap >= pr["ML"] else "layers"), "birth", normal=0.3)
    add("death_last", random_state(pr, rs, n=1), ("rule", "death_last"), "death")
    if cap >= 4:                         # the first nucleus lands between the last two
        st = random_state(pr, rs, n=min(cap, 6))
        z = st["z"]
        add("jump", st, ("note", "jump"), "zvmod", u_index=0.0, normal=((z[-2] + z[-1]) / 2 - z[0]) / st["propdist"][1])
    if cap >= 2:
        st = random_state(pr, rs, n=2)
        zb = pr["z"][0] + 0.25 * (pr["z"][1] - pr["z"][0])
        st["z"] = np.array([zb - 4.0, zb + 4.0])
        add("nearest_tie", st, ("note", "nearest_tie"), "birth", u_z=0.25, normal=0.5)
    st3 = random_state(pr, rs, n=3) if cap >= 3 else None
    ex = _exact_h(pr, st3["vs"]) if cap >= 3 else None
    if ex is not None:
        z, k = ex
        for label, zz, rule in (("h_at_thickmin", z, "ok"), ("h_below_thickmin", None, "thickmin")):
            st = copy.deepcopy(st3)
            if zz is None:
                zz = z.copy()
                zz[k + 1] = np.nextafter(zz[k + 1], 0.0)
                while get_vp_vs_h(np.ones(3), zz, 1.0, None)[2][k] >= pr["thickmin"]:
                    zz[k + 1] = np.nextafter(zz[k + 1], 0.0)
            st["z"] = zz
            add(label, st, ("rule", rule), "vsmod")
    if cap >= 2:
        for name, f in (("lvz", lambda v: v * (1 - pr["lvz"])), ("hvz", lambda v: v * (1 + pr["hvz"]))):
            if pr[name] is None:
                continue
            vi = np.float64(pr["vs"][1] * 0.93 if name == "lvz" else pr["vs"][0] * 1.05)
            inward = np.inf if name == "lvz" else -np.inf
            for label, vn, rule in ((name + "_zero", f(vi), name), (name + "_one_ulp_inside", np.nextafter(f(vi), inward), "ok")):
                if not pr["vs"][0] <= vn <= pr["vs"][1]:
                    continue
                st = random_state(pr, rs, n=max(2, nmin))    # (equal velocities above: they pass lvz and hvz)
                st["vs"] = np.concatenate((np.full(st["n"] - 1, vi), [vn]))
                add(label, st, ("rule", rule), "vsmod")
    ni = noiseinds(pr)
    if len(ni) >= 2:                     # the picked parameter stays inside, another free one is outside already
        st = random_state(pr, rs)
        st["noise"][ni[-1]] = pr["noise_hi"][ni[-1]] * 2 + 1.0
        add("noise_other", st, ("note", "noise_other"), "noise", u_noise=0.0)
    if pr["mantle"] is not None and cap >= 3 and (pr["lvz"] is None or pr["lvz"] >= 0.1):
        m = pr["mantle"][0]
        st = random_state(pr, rs, n=3)
        st["vs"] = np.array([m - 0.3, m + 0.1, m - 0.1])
        add("sticky_mantle", st, ("note", "sticky_mantle"), "vpvs" if _u_for("vpvs", pr, iiter) else "vsmod")
    for name, u in (("zero", 0.0), ("top", TOP), ("one", 1.0)):
        expect = ("note", {"zero": "%s_first", "top": "%s_last", "one": "%s_clamp"}[name])
        add("u_move_" + name, random_state(pr, rs), (expect[0], expect[1] % "move"), None, u_move=u, normal=0.1)
        add("u_index_" + name, random_state(pr, rs, n=cap), ("note", "index_clamp" if name == "one" else
                                                               ("index_last" if name == "top" else "index_inner")),
            "vsmod", u_index=u, normal=0.1)
        add("u_noise_" + name, random_state(pr, rs), (expect[0], expect[1] % "noise"), "noise", u_noise=u, normal=0.1)
    # a parameter exactly on its bound, and one ulp outside (normal = 0: the state itself is the proposal)
    for label, v, rule in (("vs_on_bound", pr["vs"][1], "ok"), ("vs_one_ulp_out", np.nextafter(pr["vs"][1], np.inf), "vs")):
        st = random_state(pr, rs, n=min(cap, max(2, nmin)))  # (one nucleus: its interface at depth 0 fails a zmin > 0)
        st["vs"] = v * 0.9 ** np.arange(st["n"] - 1, -1, -1)   # (steps that pass lvz and hvz)
        add(label, st, ("rule", rule), "zvmod")
    if pr["vpvs"][0] != pr["vpvs"][1]:
        for label, v, rule in (("vpvs_on_bound", pr["vpvs"][0], "ok"), ("vpvs_one_ulp_out", np.nextafter(pr["vpvs"][0], 0), "vpvs")):
            st = random_state(pr, rs)
            st["vpvs"] = v
            add(label, st, ("rule", rule), "vpvs")
    if len(ni):
        k = ni[0]
        for label, v, rule in (("noise_on_bound", pr["noise_hi"][k], "ok"), ("noise_one_ulp_out", np.nextafter(pr["noise_hi"][k], 9.), "noise")):
            st = random_state(pr, rs)
            st["noise"][k] = v
            add(label, st, ("rule", rule), "noise", u_noise=0.0)
    return out


# what the population of one usual record (records()[0]) must contain once the early phase is over, and what the early phase allows
PROPOSE_BRANCHES = ("birth_full", "death_last", "jump", "nearest_tie", "h_at_thickmin", "h_below_thickmin", "lvz_zero",
                    "lvz_one_ulp_inside", "noise_other", "sticky_mantle", "u_move_zero", "u_move_top", "u_move_one", "u_index_zero",
                    "u_index_top", "u_index_one", "u_noise_zero", "u_noise_top", "u_noise_one", "vs_on_bound", "vs_one_ulp_out",
                    "vpvs_on_bound", "vpvs_one_ulp_out", "noise_on_bound", "noise_one_ulp_out")
EARLY_EXCLUDED = ("birth_full", "death_last", "nearest_tie")


def population(kind, C, ML, nt, depth, iiter, seed=0):
    """Crafted chains for the propose kernels.  kind: 'plain' (record 0 for every chain), 'variant' (record 1: zmin > 0, no
    mantle, no lvz, ...), 'absent' (record 0 and an absent mask per chain), 'priors' (the four records scattered over the chains,
    some chains with a record index out of range).  `recs` always holds four records: four copies of the one in use where the
    kind has no table, so that a 'plain' population can be put through the builds with a table as well.
    -> dict: states[C], priors[C] (each chain's own dict), recs, prior_of[C], absent[C], draws[depth, 6, C],
             designed = [(chain, label, expect)], iiter, depth"""
    rs = np.random.RandomState(1000 * seed + 31 * ML + 7 * nt + depth + (17 if iiter < 0 else 0) + len(kind))
    recs = records(nt, ML)
    if kind in ("plain", "absent"):
        recs = [recs[0]] * 4
    elif kind == "variant":
        recs = [recs[1]] * 4
    prior_of = np.array([(c * 5 + c // 4) % 4 for c in range(C)], dtype=np.int32)
    if kind == "priors":
        prior_of[0] = 1                  # the birth with no room left, under the record whose layers max + 1 < ML
    absent = np.zeros(C, dtype=np.uint8)
    if kind in ("absent", "priors"):
        absent = rs.randint(0, 1 << nt, C).astype(np.uint8)
        absent[::3] = 0
    bad = np.zeros(C, dtype=bool)
    if kind == "priors":
        bad[[C - 1, C // 2, 5]] = True
    draws = np.empty((depth, 6, C))
    draws[:, :5], draws[:, 5] = rs.uniform(size=(depth, 5, C)), rs.normal(size=(depth, C))
    for k, u in ((0, 0.0), (1, TOP), (2, 1.0)):      # the clamps at every level of some chains
        c = C - 2 - k
        draws[:, (0, 1, 4), c] = u
    draws[depth - 1, 0, C - 5], draws[depth - 1, 5, C - 5] = 0.0, 1e3     # an invalid proposal at the window's last iteration
    priors, states, designed = [], [], []
    crafted = {}
    for c in range(C):
        pr = dict(recs[prior_of[c]], absent=int(absent[c]), bad=bool(bad[c]))
        key = (int(prior_of[c]), int(absent[c]))
        if key not in crafted:
            crafted[key] = crafted_propose(pr, iiter, np.random.RandomState(rs.randint(1 << 30)))
        priors.append(pr)
        cases = crafted[key]
        i = c % 33                       # chain c takes case c mod 33 of its own record's list, while that list lasts
        if not bad[c] and c < C - 4 and i < len(cases):
            label, st, d6, expect = cases[i]
            states.append(copy.deepcopy(st))
            draws[0, :, c] = d6
            designed.append((c, label, expect))
            continue
        states.append(random_state(pr, rs, wide=bool(c % 2)))
    po = prior_of.copy()
    if kind == "priors":
        po[C - 1], po[C // 2], po[5] = 4, -1, 1 << 20
    return dict(states=states, priors=priors, recs=recs, prior_of=po, absent=absent, draws=draws, designed=designed, iiter=iiter,
                depth=depth, C=C, ML=ML, nt=nt, kind=kind)


def trees(pop):
    return [window(pop["states"][c], pop["priors"][c], pop["draws"][:, :, c], pop["iiter"], pop["depth"]) for c in range(pop["C"])]


def accept_population(pop, tr, seed=0, beta=False):
    """Synthetic logL / misfits over the trees `tr` of `pop`, the acceptance draws and the counters of every chain, crafted by
    chain index.  -> dict: logL[N, C], misfits[N, C, nt+1], draws (a copy of pop's with u_accept set), states (copies with
    like, counters and widths set), beta[C] or None, designed = [(chain, label)], trees (tr, changed in place: the trees of the
    chains whose widths were set)
    The path of a chain does not depend on its counters, so counters are set AFTER a first walk: the final counts are chosen
    and the walk's increments subtracted."""
    C, depth, nt, iiter = pop["C"], pop["depth"], pop["nt"], pop["iiter"]
    N = (1 << depth) - 1
    rs = np.random.RandomState(77 + seed + depth + C)
    states = copy.deepcopy(pop["states"])
    draws = pop["draws"].copy()
    draws[:, 3, :] = rs.uniform(size=(depth, C))
    betas = rs.uniform(0.05, 1.0, C) if beta else None
    if beta:
        betas[::5] = 1.0
    logL = np.zeros((N, C))
    misfits = rs.uniform(0, 2, (N, C, nt + 1))
    designed = []
    labels = ("nan", "tie_u1", "tie_u0", "all_rejected", "all_accepted", "just_above", "just_below", "on_lo", "on_hi", "floor",
              "zero_proposed", "below", "above", "inside")
    for c in range(C):
        st = states[c]
        cur = st["like"]
        logL[:, c] = cur + rs.normal(size=N) * 1.5
        label = labels[c % len(labels)]
        if label == "floor":              # (the widths enter the proposals: this chain's tree is made again)
            st["propdist"] = np.array([0.00104, 0.001, 0.002, 0.00105, 0.0010526])
            tr[c] = window(st, pop["priors"][c], draws[:, :, c], iiter, depth)
        if label == "nan":
            logL[:, c] = np.nan
        elif label in ("tie_u1", "tie_u0"):
            logL[:, c] = cur
            draws[:, 3, c] = 1.0 if label == "tie_u1" else 0.0
            for j in range(N):                      # a tie of alpha with log(1) = 0 needs alpha = dl = 0: no birth/death term
                if tr[c]["nodes"][j]["move"] in (2, 3) and label == "tie_u1":
                    logL[j, c] = cur - 1e6
        elif label == "all_rejected":
            logL[:, c] = cur - 1e6
        elif label == "all_accepted":
            logL[:, c] = cur + 1e6 * (1 + np.arange(N))
        elif label in ("just_above", "just_below") and tr[c]["nodes"][0]["valid"]:
            p = tr[c]["nodes"][0]
            u = draws[0, 3, c]
            b = None if betas is None else betas[c]
            dv = np.float64(pop["priors"][c]["vs"][1]) - np.float64(pop["priors"][c]["vs"][0])
            _, A, B, _ = acceptance_probability(MOVES[p["move"]], cur, cur, st["propdist"][2], p["dvs2"], dv, b)
            want = np.log(u) * (1 - 1e-9 if label == "just_above" else 1 + 1e-9) - (np.log(A) if A is not None else 0.0) - B
            logL[0, c] = cur + (want if b is None else want / b)
        designed.append((c, label))
    # counters: final counts chosen, the walk's own increments taken off
    for c in range(C):
        st = states[c]
        b = None if betas is None else betas[c]
        s1, _, _ = accept(st, tr[c], logL[:, c], misfits[:, c], draws[:, :, c], iiter, depth, b)
        inc_p, inc_a = s1["proposed"], s1["accepted"]
        lo, hi = pop["priors"][c]["acceptance"]
        label = labels[c % len(labels)]
        fp = np.full(5, 200.0)
        fa = np.round(rs.uniform(0, 200, 5))
        if label == "on_lo":
            fa[:] = 2 * lo
        elif label == "on_hi":
            fa[:] = 2 * hi
        elif label == "floor":
            fa[:] = 0.0
        elif label == "zero_proposed":
            fp[4] = 0.0
            fa[4] = 0.0
        elif label == "below":
            fa[:] = np.floor(2 * lo) - 1
        elif label == "above":
            fa[:] = np.ceil(2 * hi) + 1
        elif label == "inside":
            fa[:] = lo + hi
        elif c % 4 == 3:
            fp[:] = fa[:] = 0.0                     # a fresh chain
        st["proposed"] = np.maximum(fp - inc_p, 0.0)
        st["accepted"] = np.maximum(np.minimum(fa, fp) - inc_a, 0.0)
        st["naccepted"] = int(rs.randint(0, 1000)) + (1 << 33) * (c % 2)
    return dict(logL=logL, misfits=misfits, draws=draws, states=states, beta=betas, designed=designed, trees=tr)


# ---------------------------------------------------------------------------------------------------------------------------
# What tests/test_gpu_chain_kernels.py runs; tests/test_chain_ref.py checks the same populations from the reference alone.
GPU_SHAPES = ((4, 1), (21, 3), (32, 8))
GPU_PARAMS = [(C, ML, nt, depth, wide) for C in (37, 70) for ML, nt in GPU_SHAPES
              for depth, wide in ((1, False), (1, True), (2, False), (3, True), (5, False), (7, True)) if not (depth == 7 and C == 70)]
LATE = 201                               # an iteration after the early phase, no adaptation within seven iterations


def crossing(depth):
    """the first iteration of a window that crosses the early-phase boundary at -987 (depth 1: the last early iteration)"""
    return -987 - max(1, depth // 2)


def propose_populations(C, ML, nt, depth):
    """-> [(build, population)]: build 'plain', 'absent' or 'priors'"""
    return [("plain", population("plain", C, ML, nt, depth, LATE)), ("plain", population("variant", C, ML, nt, depth, crossing(depth))),
            ("absent", population("absent", C, ML, nt, depth, LATE)), ("priors", population("priors", C, ML, nt, depth, LATE)),
            ("priors", population("priors", C, ML, nt, depth, crossing(depth)))]


def accept_populations(C, ML, nt, depth):
    """-> [(build, population, with beta)]: the window's last iteration is 1000 or -1000 (adaptation) or none is"""
    return [("plain", population("plain", C, ML, nt, depth, 1000 - (depth - 1)), False),
            ("plain", population("plain", C, ML, nt, depth, -1000 - (depth - 1), seed=1), True),
            ("priors", population("priors", C, ML, nt, depth, 1000 - (depth - 1), seed=2), True),
            ("priors", population("priors", C, ML, nt, depth, LATE, seed=3), False)]


ACCEPT_NOTES = ("adapt", "below", "inside", "above", "on_band", "floor", "zero_proposed", "invalid_at_adapt", "unchanged")


def walk(pop, tr, ap):
    """accept() for every chain of a population -> [(state, decisions, notes)]"""
    return [accept(ap["states"][c], tr[c], ap["logL"][:, c], ap["misfits"][:, c], ap["draws"][:, :, c], pop["iiter"], pop["depth"],
                   None if ap["beta"] is None else ap["beta"][c]) for c in range(pop["C"])]
