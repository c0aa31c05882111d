"""The four chain-step kernels of csrc/chain_kernel.hip in their three builds (plain, BH_CHAIN_ABSENT, BH_CHAIN_PRIORS), called
directly and compared decision by decision with tests/chain_ref.py -- the plain restatement of the reference's step, pinned to
the reference in tests/test_chain_ref.py.  No forward model: the kernels read and write plain arrays, logL / misfits are synthetic.

  proposals   bit for bit on every REACHABLE node of the window's tree (move, valid, dvs2, the proposal, the layered model);
              an unreachable node (below the "accepted" edge of an invalid proposal) must only be well formed for the evaluate call
  accept      a chain counts if every decision of its walk is further from its threshold than the rounding budget of the double
              evaluation, 64 * 2^-53 * (|log A| + |B| + |dl| + |log u|) (chain_ref.margin, mpmath); then state, counters and
              adapted widths bit for bit.  tests/test_chain_ref.py shows that no population leaves a chain out.
  draws       inject = NULL: Philox words and their mapping exact (through integers and through u_z itself), the Box-Muller
              deviate against mpmath from the exact words
Shapes: C = 37 and 70 (no multiple of any 64 >> (depth - 1)), (ML, nt) = (4, 1), (21, 3), (32, 8) -- the last is the header's limit
and the big-LDS path of the window kernel from depth 5 on --, depth 1 (lane kernel), 1 with ld > C (window kernel, T = 1), 2, 3, 5, 7.
"""
import ctypes

import mpmath
import numpy as np
import pytest

import chain_ref as R
from bayhunter_amd import engine as E
from philox_ref import philox4x32_10, draws as philox_draws

pytestmark = pytest.mark.gpu

PROPOSAL = ("move", "valid", "dvs2", "pn", "pvs", "pz", "pvpvs", "pnoise", "lay_n", "lay_h", "lay_vs", "lay_vp", "lay_rho")
STATE = ("n", "vs", "z", "vpvs", "noise", "like", "misfits", "propdist", "proposed", "accepted", "naccepted")


def station_fields(o, pr):
    """the station's entries of a ChainConfig or a ChainPrior"""
    nt = pr["nt"]
    o.layermin, o.layermax = pr["layers"]
    o.vsmin, o.vsmax = pr["vs"]
    o.zmin, o.zmax = pr["z"]
    o.thickmin = pr["thickmin"]
    o.lvz = -1.0 if pr["lvz"] is None else pr["lvz"]
    o.hvz = -1.0 if pr["hvz"] is None else pr["hvz"]
    o.vpvsmin, o.vpvsmax = pr["vpvs"]
    o.mantle_vs, o.mantle_vpvs = (-1.0, 0.0) if pr["mantle"] is None else pr["mantle"]
    o.acc_lo, o.acc_hi = pr["acceptance"]
    for i in range(2 * nt):
        o.noise_lo[i], o.noise_hi[i] = pr["noise_lo"][i], pr["noise_hi"][i]


def make_cfg(pr, ML, own=True, seed=0, offset=0):
    """own = False: the station's entries hold nonsense -- the builds with a table must not read them"""
    cfg = E.ChainConfig()
    if own:
        station_fields(cfg, pr)
    else:
        station_fields(cfg, R.make_priors(pr["nt"], ML, layers=(7, 3), vs=(9., 1.), z=(9., 1.), thickmin=99., lvz=5., hvz=5., vpvs=(3., 1.),
                                          mantle=(0.1, 9.), acceptance=(99., 1.)))
    cfg.nt, cfg.maxlayers, cfg.iter_burnin, cfg.iterations = pr["nt"], ML, pr["iter_burnin"], pr["iterations"]
    cfg.seed, cfg.chain_offset = seed, offset
    return cfg


class Device(object):
    """hand-built chain state over torch tensors; arrays the kernels write start from values they never produce"""

    def __init__(self, eng, states, ML, nt, depth, wide, inject, beta=None):
        import torch
        self.torch, self.eng = torch, eng
        C = self.C = len(states)
        self.ML, self.nt, self.depth = ML, nt, depth
        N = self.N = (1 << depth) - 1
        self.ld = N * C + (11 if wide else 0)
        dev = torch.device("cuda", 0)
        h = {}
        h["n"] = np.array([s["n"] for s in states], dtype=np.int32)
        h["vs"], h["z"] = np.zeros((ML, C)), np.zeros((ML, C))
        for c, s in enumerate(states):
            h["vs"][:s["n"], c], h["z"][:s["n"], c] = s["vs"], s["z"]
        h["vpvs"] = np.array([s["vpvs"] for s in states], dtype=float)
        h["noise"] = np.array([s["noise"] for s in states], dtype=float).T.copy()
        h["like"] = np.array([s["like"] for s in states], dtype=float)
        h["misfits"] = np.array([s["misfits"] for s in states], dtype=float).T.copy()
        for k in ("propdist", "proposed", "accepted"):
            h[k] = np.array([s[k] for s in states], dtype=float).T.copy()
        h["naccepted"] = np.array([s["naccepted"] for s in states], dtype=np.int64)
        self.host0 = h
        t = {k: torch.from_numpy(v).to(dev) for k, v in h.items()}
        t["beta"] = None if beta is None else torch.from_numpy(np.asarray(beta, dtype=float)).to(dev)
        f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
        for k in ("pn", "move", "valid", "lay_n"):
            t[k] = torch.full((self.ld,), -77, **i32)
        for k in ("pvs", "pz", "lay_h", "lay_vp", "lay_vs", "lay_rho"):
            t[k] = torch.full((ML, self.ld), float("nan"), **f64)
        t["pvpvs"], t["dvs2"] = torch.full((self.ld,), float("nan"), **f64), torch.full((self.ld,), float("nan"), **f64)
        t["pnoise"] = torch.full((self.ld, 2 * nt), float("nan"), **f64)
        t["inject"] = None if inject is None else torch.from_numpy(np.ascontiguousarray(inject, dtype=float)).to(dev)
        self.t = t
        self.state = E.ChainState()
        for k, _ in E.ChainState._fields_:
            setattr(self.state, k, None if t[k] is None else t[k].data_ptr())
        torch.cuda.synchronize(dev)

    def upload(self, a, dtype=None):
        x = self.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.torch.device("cuda", 0))
        self.torch.cuda.synchronize()
        return x

    def host(self, names):
        self.eng.synchronize()
        return {k: self.t[k].cpu().numpy() for k in names}

    def columns(self, a):
        """[N, C, ...] per node and chain -> [ld, ...] in the kernels' column order (node j of chain c: column j * C + c)"""
        out = np.zeros((self.ld,) + a.shape[2:])
        out[:self.N * self.C] = a.reshape((self.N * self.C,) + a.shape[2:])
        return out


def table(dv, recs):
    arr = (E.ChainPrior * len(recs))()
    for r, pr in zip(arr, recs):
        station_fields(r, pr)
    return dv.upload(np.frombuffer(bytes(arr), dtype=np.uint8).copy())


def run_propose(eng, dv, build, pop, recs=None, prior_of=None, absent=None):
    """one propose launch of the given build; -> the proposal arrays on the host"""
    C, ML, depth = dv.C, dv.ML, dv.depth
    keep = []
    if build == "plain":
        eng.chain_propose_window(make_cfg(pop["priors"][0], ML), dv.state, C, pop["iiter"], depth, dv.ld)
    elif build == "absent":
        keep.append(dv.upload(pop["absent"] if absent is None else absent, np.uint8))
        eng.chain_propose_window(make_cfg(pop["priors"][0], ML), dv.state, C, pop["iiter"], depth, dv.ld, absent=keep[0].data_ptr())
    else:
        recs = pop["recs"] if recs is None else recs
        keep += [table(dv, recs), dv.upload(pop["prior_of"] if prior_of is None else prior_of, np.int32),
                 dv.upload(pop["absent"] if absent is None else absent, np.uint8)]
        eng.chain_propose_window_priors(make_cfg(pop["priors"][0], ML, own=False), dv.state, C, pop["iiter"], depth, dv.ld,
                                        keep[0].data_ptr(), len(recs), keep[1].data_ptr(), absent=keep[2].data_ptr())
    return dv.host(PROPOSAL)


def bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def check_tree(out, pop, tr, ML, nt, what):
    """the kernel's tree against chain_ref.window on the reachable nodes; well-formedness everywhere"""
    C, N = pop["C"], (1 << pop["depth"]) - 1
    reached = 0
    for c in range(C):
        for j, q in enumerate(tr[c]["nodes"]):
            col, w = j * C + c, what + (c, j, q["rule"])
            n = int(out["lay_n"][col])
            assert 1 <= n <= ML and out["valid"][col] in (0, 1) and out["pn"][col] == n, w
            for k in ("lay_h", "lay_vs", "lay_vp", "lay_rho", "pvs", "pz"):
                assert np.all(np.isfinite(out[k][:n, col])), w + (k,)
            assert np.all(np.isfinite(out["pnoise"][col])) and np.isfinite(out["pvpvs"][col]), w
            if pop["priors"][c]["bad"]:
                assert out["valid"][col] == 0, w
            if not q["reachable"]:
                continue
            reached += 1
            assert out["valid"][col] == int(q["valid"]), w
            if q["move"] < 0 or "equal_depths" in q["notes"]:      # a record out of range | the reference's sort is not stable there
                continue
            assert out["move"][col] == q["move"] and n == q["n"], w + (int(out["move"][col]), n)
            assert bits(out["dvs2"][col], q["dvs2"]), w + ("dvs2", out["dvs2"][col], q["dvs2"])
            for k, ref in (("pvs", q["vs"]), ("pz", q["z"]), ("lay_h", q["h"]), ("lay_vs", q["vs"]), ("lay_vp", q["vp"]), ("lay_rho", q["rho"])):
                assert bits(out[k][:n, col], ref), w + (k, out[k][:n, col], ref)
            assert bits(out["pvpvs"][col], q["vpvs"]) and bits(out["pnoise"][col], q["noise"]), w
    assert reached >= C * pop["depth"] and (N == 1 or reached > C * pop["depth"])        # (the all-rejected paths, and more)
    # nothing past the N * C columns of the call was written
    assert np.all(out["lay_n"][N * C:] == -77) and np.all(np.isnan(out["lay_h"][:, N * C:])), what


@pytest.mark.parametrize("C,ML,nt,depth,wide", R.GPU_PARAMS)
def test_proposals_of_all_three_builds(engine, C, ML, nt, depth, wide):
    """Every build on its populations (chain_ref.propose_populations: the crafted branches, the clamps of u_move / u_index /
    u_noise, a window across the early-phase boundary, zmin > 0, no mantle, no lvz, fixed vp/vs, interleaved noise slots, four
    records that differ in every field and record indices out of range) against the reference's tree; and the builds with a table
    of identical records and nothing absent against the plain build, every byte."""
    plain = None
    for build, pop in R.propose_populations(C, ML, nt, depth):
        dv = Device(engine, pop["states"], ML, nt, depth, wide, pop["draws"])
        out = run_propose(engine, dv, build, pop)
        check_tree(out, pop, R.trees(pop), ML, nt, (build, pop["kind"], pop["iiter"]))
        if pop["kind"] == "plain":
            plain = (pop, out)
    pop, out = plain
    for build in ("absent", "priors"):
        dv = Device(engine, pop["states"], ML, nt, depth, wide, pop["draws"])
        same = run_propose(engine, dv, build, pop, recs=[pop["priors"][0]] * 4, absent=np.zeros(C, dtype=np.uint8))
        for k in PROPOSAL:
            assert np.array_equal(same[k], out[k], equal_nan=True) and same[k].tobytes() == out[k].tobytes(), (build, k)


def check_states(dv, res, what):
    got = dv.host(STATE)
    ML, nt = dv.ML, dv.nt
    for c, (s, dec, notes) in enumerate(res):
        w = what + (c, sorted(notes))
        assert R.counted(dec), w                                     # (tests/test_chain_ref.py: no chain is left out)
        vs, z = np.zeros(ML), np.zeros(ML)
        vs[:s["n"]], z[:s["n"]] = s["vs"], s["z"]
        assert got["n"][c] == s["n"] and got["naccepted"][c] == s["naccepted"], w + (int(got["n"][c]), s["n"])
        for k, ref in (("vs", vs), ("z", z), ("noise", s["noise"]), ("misfits", s["misfits"]), ("propdist", s["propdist"]),
                       ("proposed", s["proposed"]), ("accepted", s["accepted"])):
            assert bits(got[k][:, c], ref), w + (k, got[k][:, c], ref)
        assert bits(got["vpvs"][c], s["vpvs"]) and bits(got["like"][c], s["like"]), w
        if "unchanged" in notes:                                      # nothing accepted: the model as it was, byte for byte
            for k in ("n", "vs", "z", "vpvs", "noise", "like", "misfits"):
                a = dv.host0[k][..., c]
                assert np.asarray(got[k][..., c]).tobytes() == np.asarray(a).tobytes(), w + (k,)


@pytest.mark.parametrize("C,ML,nt,depth,wide", R.GPU_PARAMS)
def test_accept_walks_the_reference_path(engine, C, ML, nt, depth, wide):
    """Plain and priors builds, lane kernel (depth 1) and window kernel, over the tree the propose kernel made: synthetic logL with
    NaN, exact ties at u = 1 and u = 0, all rejected / all accepted (depth 7: node 63 in the low, nodes from 64 in the high
    register), decisions 1e-9 relative either side of the threshold, beta NULL and in (0, 1], adaptation at 1000 and -1000 with
    rates below, inside, above and on the band, the 0.001 floor, a zero `proposed`, an invalid proposal at the adaptation
    iteration; chains whose record index is out of range keep their state."""
    for build, pop, beta in R.accept_populations(C, ML, nt, depth):
        tr = R.trees(pop)
        ap = R.accept_population(pop, tr, beta=beta)
        res = R.walk(pop, tr, ap)
        dv = Device(engine, ap["states"], ML, nt, depth, wide, ap["draws"], beta=ap["beta"])
        pop2 = dict(pop, states=ap["states"], draws=ap["draws"])
        out = run_propose(engine, dv, build, pop2)
        for c in range(C):                                            # the tree the walk is about to read is the reference's
            for j, q in enumerate(tr[c]["nodes"]):
                if q["reachable"]:
                    assert out["valid"][j * C + c] == int(q["valid"]) and (q["move"] < 0 or out["move"][j * C + c] == q["move"])
        logL = dv.upload(dv.columns(ap["logL"]))
        mis = dv.upload(dv.columns(ap["misfits"]))
        what = (build, pop["iiter"], beta)
        if build == "plain":
            engine.chain_accept_window(make_cfg(pop["priors"][0], ML), dv.state, C, pop["iiter"], depth, dv.ld, logL.data_ptr(),
                                       mis.data_ptr())
        else:
            tab, po = table(dv, pop["recs"]), dv.upload(pop["prior_of"], np.int32)
            engine.chain_accept_window_priors(make_cfg(pop["priors"][0], ML, own=False), dv.state, C, pop["iiter"], depth, dv.ld,
                                              logL.data_ptr(), mis.data_ptr(), tab.data_ptr(), len(pop["recs"]), po.data_ptr())
        check_states(dv, res, what)


def test_adaptation_inside_a_window_is_refused(engine):
    """an iteration with iiter % 1000 == 0 must be the last of its window: BH_EINVAL from every entry, nothing launched"""
    pop = R.population("plain", 37, 4, 1, 2, 1000)
    dv = Device(engine, pop["states"], 4, 1, 2, False, pop["draws"])
    cfg, L = make_cfg(pop["priors"][0], 4), engine._L
    buf = dv.upload(np.zeros((dv.ld, 2)))
    ab, po, tab = dv.upload(np.zeros(37), np.uint8), dv.upload(np.zeros(37), np.int32), table(dv, pop["recs"])
    for iiter, rc in ((1000, E.BH_EINVAL), (-1000, E.BH_EINVAL), (0, E.BH_EINVAL), (999, E.BH_OK), (-1001, E.BH_OK)):
        a = (engine.stream, ctypes.byref(cfg), ctypes.byref(dv.state), 37, iiter, 2, dv.ld)
        assert L.bh_chain_propose_window(*a) == rc, iiter
        assert L.bh_chain_propose_window_sites(*a, ab.data_ptr()) == rc, iiter
        assert L.bh_chain_propose_window_priors(*a, tab.data_ptr(), 4, po.data_ptr(), None) == rc, iiter
        assert L.bh_chain_accept_window(*a, buf.data_ptr(), buf.data_ptr()) == rc, iiter
        assert L.bh_chain_accept_window_priors(*a, buf.data_ptr(), buf.data_ptr(), tab.data_ptr(), 4, po.data_ptr()) == rc, iiter
        engine.synchronize()


# ---- the device's own draws (inject = NULL) -------------------------------------------------------------------------------
SEED, OFFSET = (0x5eed1234 << 32) | 0x9abcdef1, 300


def words(seed, C, iiter, offset, purpose):
    ctr = np.zeros((C, 4), dtype=np.uint32)
    ctr[:, 0] = (np.arange(C, dtype=np.uint64) + np.uint64(offset)).astype(np.uint32)
    ctr[:, 1], ctr[:, 2] = np.uint32(iiter & 0xFFFFFFFF), purpose
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def mp_normal(w):
    """Box-Muller at 50 digits from the four exact words of purpose 3"""
    with mpmath.workdps(50):
        a = 1 - mpmath.mpf(int((int(w[0]) << 32 | int(w[1])) >> 11)) / 2 ** 53
        b = mpmath.mpf(int((int(w[2]) << 32 | int(w[3])) >> 11)) / 2 ** 53
        return mpmath.sqrt(-2 * mpmath.log(a)) * mpmath.cos(2 * mpmath.pi * b)


def wide_priors(nt, ML, **kw):
    return R.make_priors(nt, ML, layers=(0, ML - 1), vs=(-1e3, 1e3), z=(-1e3, 1e3), thickmin=-1.0, lvz=None, hvz=None, vpvs=(1.7, 1.7),
                         mantle=None, **kw)


def flat_state(pr, n, vs, z):
    nt = pr["nt"]
    return dict(n=n, vs=np.array(vs, dtype=float), z=np.array(z, dtype=float), vpvs=1.7, noise=0.5 * (pr["noise_lo"] + pr["noise_hi"]),
                like=0.0, misfits=np.zeros(nt + 1), propdist=np.ones(5), proposed=np.zeros(5), accepted=np.zeros(5), naccepted=0)


def test_device_normal_deviate_against_mpmath(engine):
    """Early phase, one nucleus at vs = z = 0, width 1, nothing else free: every proposal is 0 + normal on vs or z.  Depth 3: level
    k must use the draws of iteration iiter + k.  Measured on the MI355X: the largest distance from the mpmath value over these
    2700 deviates is 1.902 ulp; asserted: the next power of two, 2 ulp.  (More than 8 ulp would be a finding, not a tolerance:
    1 for log, a correctly rounded sqrt, 2 for cospi, the product, and slack.)"""
    C, ML, nt, depth = 300, 4, 1, 3
    pr = wide_priors(nt, ML)
    states = [flat_state(pr, 1, [0.0], [0.0]) for _ in range(C)]
    worst, count = 0.0, 0
    for iiter in (-999, -995, -991):                                 # (all early: before -987; negative: counter words above 2^31)
        dv = Device(engine, states, ML, nt, depth, False, None)
        engine.chain_propose_window(make_cfg(pr, ML, seed=SEED, offset=OFFSET), dv.state, C, iiter, depth, dv.ld)
        out = dv.host(PROPOSAL)
        for k in range(depth):
            w = words(SEED, C, iiter + k, OFFSET, 3)
            um = philox_draws(SEED, C, iiter + k, OFFSET)[0]
            j = (1 << k) - 1                                          # the all-rejected node of level k: proposed from the state
            for c in range(C):
                col = j * C + c
                move = int(um[c] * 2)
                assert out["valid"][col] == 1 and out["move"][col] == move, (iiter, k, c)
                got = out["pvs" if move == 0 else "pz"][0, col]
                ref = mp_normal(w[c])
                d = abs(float((mpmath.mpf(float(got)) - ref) / mpmath.mpf(float(np.spacing(abs(float(ref)))))))
                worst, count = max(worst, d), count + 1
    print("normal deviate: largest distance from mpmath %.3f ulp over %d deviates" % (worst, count))
    assert worst <= 2.0 and count == 3 * 3 * C


def test_device_uniform_draws_are_the_philox_words(engine):
    """u_z itself through a birth between z = 0 and 1; u_move, u_index and u_noise through the integers they select, over more
    than 10^4 (chain, iteration) pairs; a seed with a high word, chain_offset 300, negative iterations."""
    C, ML, nt = 520, 8, 8
    lo, hi = np.zeros(2 * nt), np.ones(2 * nt)
    pr = R.make_priors(nt, ML, layers=(0, ML - 1), vs=(-1e3, 1e3), z=(0.0, 1.0), thickmin=-1.0, lvz=None, hvz=None, vpvs=(1.0, 3.0),
                       mantle=None, noise_lo=lo, noise_hi=hi)
    st = flat_state(pr, 4, [1.0, 2.0, 3.0, 4.0], [0.1, 0.3, 0.5, 0.7])
    one = flat_state(pr, 1, [1.0], [0.0])
    states = [st if c % 2 else one for c in range(C)]
    pairs = 0
    for iiter in list(range(-910, -900)) + list(range(5, 15)):
        dv = Device(engine, states, ML, nt, 1, bool(iiter % 2), None)
        engine.chain_propose_window(make_cfg(pr, ML, seed=SEED, offset=OFFSET), dv.state, C, iiter, 1, dv.ld)
        out = dv.host(PROPOSAL)
        d = philox_draws(SEED, C, iiter, OFFSET)
        move = np.minimum((d[0] * 6).astype(int), 5)
        assert np.array_equal(out["move"][:C], move), iiter
        for c in range(C):
            n = states[c]["n"]
            if move[c] in (0, 1) and n == 4:                          # which nucleus: u_index
                a = out["pvs" if move[c] == 0 else "pz"][:n, c]
                b = states[c]["vs" if move[c] == 0 else "z"]
                changed = np.flatnonzero(a != b)
                if move[c] == 0:                                      # (a moved depth is re-sorted: only vs shows the index in place)
                    assert list(changed) == [int(d[1][c] * 4)], (iiter, c)
            elif move[c] == 2 and n == 1 and out["valid"][c]:         # the new nucleus sits at u_z exactly
                assert out["pn"][c] == 2 and out["pz"][1, c] == d[2][c], (iiter, c)
            elif move[c] == 4:                                        # which noise parameter: u_noise
                changed = np.flatnonzero(out["pnoise"][c] != states[c]["noise"])
                assert list(changed) == [int(d[4][c] * 16)] or not out["valid"][c], (iiter, c)
            pairs += 1
    assert pairs >= 10 ** 4


def test_device_accept_draw_decides(engine):
    """logL set so that alpha = log(u_ref) * (1 -+ 1e-9) at level c mod 3 of a depth-3 window (level k: the draw of iteration
    iiter + k), everything else far below: the chain accepts exactly once, or never."""
    C, ML, nt, depth, iiter = 70, 4, 1, 3, -1000 + 3
    pr = wide_priors(nt, ML)
    states = [flat_state(pr, 1, [0.0], [0.0]) for _ in range(C)]
    dv = Device(engine, states, ML, nt, depth, True, None)
    cfg = make_cfg(pr, ML, seed=SEED, offset=OFFSET)
    engine.chain_propose_window(cfg, dv.state, C, iiter, depth, dv.ld)
    assert np.all(dv.host(PROPOSAL)["valid"][:7 * C] == 1)
    logL = np.full((7, C), -1e9)
    for c in range(C):
        k = c % 3
        u = philox_draws(SEED, C, iiter + k, OFFSET)[3][c]
        logL[(1 << k) - 1, c] = np.log(u) * (1 - 1e-9 if (c // 3) % 2 == 0 else 1 + 1e-9)
    dl, dm = dv.upload(dv.columns(logL)), dv.upload(dv.columns(np.zeros((7, C, nt + 1))))
    engine.chain_accept_window(cfg, dv.state, C, iiter, depth, dv.ld, dl.data_ptr(), dm.data_ptr())
    got = dv.host(STATE)
    assert np.array_equal(got["naccepted"], np.array([1 if (c // 3) % 2 == 0 else 0 for c in range(C)])), got["naccepted"]
    assert np.all(got["proposed"].sum(axis=0) == 3)
