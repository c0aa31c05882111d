#!/usr/bin/env python3
"""Mine tests/golden/swd_hard_golden.npz: the models of a sampler's prior on which the default dispersion path has to work for
its parity with the reference -- found on the CPU, with the oracle alone.  The engine is never imported: the prior's draw,
bayhunter_amd/synth.py (numpy only), is loaded from its file, not through the package, whose __init__ imports the engine's module.

    python tools/mine_hard_swd_models.py [--threads N] [--cache DIR] [--out FILE]

The oracle restates the engine's short refinement WITHOUT its guard (oracle.set_swd_search(1)).  A model on which that mode leaves
the reference's sequence (mode 0) is a model the guard, or the lean kernel's counting of a special cell, must catch.  Drawn are
bayhunter_amd.synth.prior_models (L = 21, 2 ... 21 layers) in chunks of CHUNK models, chunk c from RandomState(SEED + c), searched
at two period sets (PERIOD_SETS) and both wave types, and kept, in the order of the draw:

  needs_guard     mode 1 differs from mode 0 by the fuzz test's criterion (relative difference > 2.5e-6, another failure flag,
                  another zero pattern): 100 per (wave type, period set)
  close_modes     the second mode's root (oracle.swd_batch(..., mode=2)) within dc / 10 = 0.0005 km/s of the fundamental's at some
                  period: 25 per (wave type, period set)
  near_halfspace  a reference root within 1e-5 c of the half-space's S velocity (near_kind 0: 15 per wave type and period set) or,
                  where another layer is the fastest, of betmx (near_kind 1; Love only, Rayleigh has none: 20 per period set)
  control         the first 32 draws of chunk 0 per period set, unselected
  water           one of chunk 0's draws with its top layer turned into water (the lean kernel guards such a model at once)

A (wave type, period set) is no longer searched once its classes are full, and the second-mode calls stop with close_modes: the
thresholds are the issue's (tighten them if a class overflows, never loosen them).  Per kept model the file holds the model as
float64, its class, the wave type and period set it was selected under, where in the draw it came from, and FOR BOTH WAVE TYPES at
its period set: the reference's velocities and flag (mode 0), the oracle's restatement of the guarded short refinement in exact
arithmetic (mode 2) and the label fastm_differs = (mode 2 differs from mode 0 by the criterion).  At most 2 % of the set may
carry that label: of every (class, wave type, period set) the first three such candidates are kept and the others passed over (at
the irregular periods most needs_guard candidates carry it, so those searches go on until 100 without it are found).  Velocities
are kept as binary32 (what the reference returns; asserted).

EXCEPTIONS and UNEXPLAINED list the models that the GPU test moved out of its asserted set -- (chunk, index, wave type, period
index, class, the velocity the default path gave on the GPU: the only numbers here that are not the oracle's; they place the probe
and are kept as evidence) -- and the file keeps probe_cell's numbers beside them (ex_probe: the reference's root, that velocity, the
grid's start, the cell probed, the distance of the sign change nearest to a grid point from it relative to c, the distance of its
neighbouring sign change in km/s, up to six sign changes) and ex_kind: 1 where those numbers meet the criterion of the documented
exception (exception_like: a sign change within 1e-6 c of a grid point, its neighbour less than a step away), 0 where they do
not (a rule's miss: the open cases).  The miner itself never runs the engine.

The result is a function of SEED alone (threads only share the work; the archive is written with fixed time stamps): the same bytes
on every run.  --cache DIR keeps every chunk's candidate lists, so that a second run only assembles.
"""
import argparse
import io
import os
import sys
import time
import zipfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SEED = 20261020
CHUNK = 50000
MAX_CHUNKS = 80
LMAX = 21
DC = 0.005
RTOL = 2.5e-6          # tests/test_gpu_fuzz.py: beyond it a model is on another root
CLOSE = DC / 10.0      # close_modes
NEAR = 1e-5            # near_halfspace, relative
PERIOD_SETS = (np.linspace(2.0, 60.0, 30),
               np.array([1.0, 1.37, 2.05, 2.9, 3.66, 4.8, 6.1, 7.45, 9.3, 11.0, 13.7, 16.2, 19.9, 23.5, 28.1, 33.3, 39.6, 46.8, 55.2,
                         66.9, 80.0]))
KMAX = 30
WAVES = (2, 1)         # column 0: Rayleigh (iwave 2), column 1: Love (iwave 1)
CLASSES = ("control", "needs_guard", "close_modes", "near_halfspace", "water", "known_exception", "unexplained")
QUOTA = {"needs_guard": 100, "close_modes": 25, "near_hs": 15, "near_bx": 20}
# raw candidates per quota before a search is closed: a model is kept once (a root next to the half-space velocity often needs the
# guard as well, and needs_guard comes first), and the fastm_differs cap passes over some
SPARE = {"needs_guard": 1.05, "close_modes": 1.4, "near_hs": 3, "near_bx": 2}
NCONTROL = 32
FASTM_CAP = 0.02
FASTM_PER_SLOT = 3     # of a (class, wave type, period set): the first three such candidates are kept, the set's cap permitting
# Models the GPU test moved out of path (c)'s ordinary assertion: (chunk, index, iwave, period index, class, the default path's velocity
# at that period as the MI355X gave it).  All eight are the documented exception of DESIGN.md 4: probe_cell finds two sign changes
# less than a scan step apart, one of them within 1e-6 c of a point of the reference's grid -- the engine's grid, anchored at its own
# previous root (up to 2.5e-6 c from the reference's), has both in one cell where the reference's has them in two, or the other way round.
EXCEPTIONS = ((2, 10106, 2, 2, "known_exception", 2.49979567527771), (6, 4106, 2, 1, "known_exception", 3.0610218048095703),
              (10, 24200, 2, 1, "known_exception", 2.230638265609741), (3, 4524, 1, 2, "known_exception", 3.6656672954559326),
              (6, 28320, 1, 1, "known_exception", 3.0098941326141357), (1, 609, 2, 6, "known_exception", 3.600841760635376),
              (7, 8132, 1, 4, "known_exception", 3.2928168773651123), (12, 31206, 1, 4, "known_exception", 3.5884876251220703))

# Candidates that the fastm_differs cap passed over -- 318 in all, 313 of them at the irregular period set -- run once through the
# default path on the MI355X, at 64 and at 16 trials: these 43, all of the irregular set, left the reference there as well.  Kept,
# beyond the classes' sizes and outside the cap, as class unexplained with probe_cell's numbers.  By those numbers (ex_kind) 35 are
# the documented exception again -- known_exception is at its 2 % -- and 8 are not: several sign changes inside one cell away from
# the grid's points, a rule's miss whose cause is open.  The period index is the first that differs; velocities as printed (9 digits).
UNEXPLAINED = ((4, 21601, 2, 0, "unexplained", 2.32277775),
               (7, 35298, 2, 4, "unexplained", 2.53372383),
               (8, 22337, 2, 1, "unexplained", 2.70084357),
               (12, 7802, 2, 1, "unexplained", 2.41708136),
               (12, 37125, 2, 2, "unexplained", 3.47437882),
               (14, 25073, 2, 3, "unexplained", 2.51084161),
               (15, 31766, 2, 1, "unexplained", 2.37098646),
               (19, 5793, 2, 4, "unexplained", 3.42385817),
               (19, 49021, 2, 4, "unexplained", 3.8458395),
               (20, 38586, 2, 1, "unexplained", 2.2325716),
               (23, 29357, 2, 0, "unexplained", 2.16578722),
               (25, 28798, 2, 1, "unexplained", 2.42813659),
               (26, 29451, 2, 3, "unexplained", 2.77751803),
               (28, 40202, 2, 0, "unexplained", 2.34448552),
               (28, 45029, 2, 2, "unexplained", 3.07292104),
               (29, 11572, 2, 0, "unexplained", 2.42104721),
               (29, 21908, 2, 1, "unexplained", 2.7461431),
               (34, 12007, 2, 0, "unexplained", 2.07476807),
               (34, 18844, 2, 1, "unexplained", 2.55007362),
               (6, 28668, 2, 2, "unexplained", 3.16588521),
               (15, 44321, 2, 2, "unexplained", 2.48410654),
               (29, 11744, 2, 1, "unexplained", 2.5184207),
               (0, 38984, 1, 7, "unexplained", 3.33000612),
               (1, 45529, 1, 1, "unexplained", 2.58082604),
               (2, 26168, 1, 1, "unexplained", 2.86640477),
               (2, 40665, 1, 1, "unexplained", 2.10830712),
               (2, 43477, 1, 4, "unexplained", 2.64240265),
               (2, 48873, 1, 1, "unexplained", 3.32334065),
               (3, 13221, 1, 5, "unexplained", 3.47760892),
               (4, 39268, 1, 3, "unexplained", 2.8350327),
               (7, 21943, 1, 1, "unexplained", 2.08474255),
               (8, 35081, 1, 1, "unexplained", 2.51080489),
               (10, 17133, 1, 2, "unexplained", 2.90948749),
               (11, 10259, 1, 1, "unexplained", 2.23002434),
               (12, 19084, 1, 3, "unexplained", 2.85849905),
               (13, 21692, 1, 0, "unexplained", 2.0160737),
               (13, 42057, 1, 1, "unexplained", 2.18404126),
               (14, 13082, 1, 2, "unexplained", 2.75960517),
               (15, 8954, 1, 1, "unexplained", 2.66140652),
               (17, 18196, 1, 17, "unexplained", 4.21217775),
               (17, 20687, 1, 1, "unexplained", 2.40327907),
               (18, 1367, 1, 2, "unexplained", 2.97734642),
               (15, 28107, 1, 6, "unexplained", 2.62629652))


def differs(v, e, rv, re_):
    """per model: the fuzz test's criterion of being on another root than the reference's"""
    both = (v != 0) & (rv != 0)
    rel = np.zeros_like(v)
    rel[both] = np.abs(v[both] - rv[both]) / np.abs(rv[both])
    return (rel.max(axis=1) > RTOL) | (e != re_) | ((v == 0) != (rv == 0)).any(axis=1)


def _synth():
    """bayhunter_amd/synth.py loaded from its file: importing it through the package would import the engine's module too"""
    if "_bh_synth" not in sys.modules:
        import importlib.util
        spec = importlib.util.spec_from_file_location("_bh_synth", os.path.join(REPO, "bayhunter_amd", "synth.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["_bh_synth"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["_bh_synth"]


def draw(chunk):
    nlay, h, vp, vs, rho = _synth().prior_models(np.random.RandomState(SEED + chunk), CHUNK, LMAX, nmin=2)
    return nlay, np.stack([h, vp, vs, rho])


def search(O, nlay, model, periods, iwave, smode, mode=1, threads=0):
    """(vel [B, K], err [B]) of the oracle's search mode smode; model [4, L, B] layer-major"""
    a = [np.ascontiguousarray(x.T) for x in model]
    O.set_swd_search(smode)
    try:
        v, e, _ = O.swd_batch(nlay, a[0], a[1], a[2], a[3], periods, iwave, 0, mode=mode, nthreads=threads)
    finally:
        O.set_swd_search(0)
    return v, e


def near_kinds(nlay, model, v0):
    """per model: a reference root within NEAR of the half-space's S velocity (bit 0) / of a faster layer's, betmx (bit 1)"""
    vs32 = model[2].astype(np.float32).astype(np.float64)            # [L, B]: what the reference searches with
    B = nlay.size
    bh = vs32[nlay - 1, np.arange(B)]
    bx = vs32.max(axis=0)
    ok = v0 != 0
    hs = (ok & (np.abs(v0 - bh[:, None]) <= NEAR * v0)).any(axis=1)
    mx = (ok & (np.abs(v0 - bx[:, None]) <= NEAR * v0)).any(axis=1) & (bx != bh)
    return hs.astype(np.int8) | (mx.astype(np.int8) << 1)


def close_modes(v1, v2):
    ok = (v1 != 0) & (v2 != 0)
    return (ok & (np.abs(v2 - v1) < CLOSE)).any(axis=1)


def scan_chunk(O, chunk, ps, iwave, want, threads, cache):
    """candidate indices of one chunk at one period set and wave type: {"m1": needs_guard, "hs", "bx": near_halfspace, "sec":
    close_modes} for the pieces in `want` ("near" comes with the reference's run)"""
    got, missing = {}, []
    for piece in want:
        f = cache and os.path.join(cache, "s%d_c%03d_p%d_w%d_%s.npy" % (SEED, chunk, ps, iwave, piece))
        if f and os.path.exists(f):
            got[piece] = np.load(f)
        else:
            missing.append((piece, f))
    if missing:
        nlay, model = draw(chunk)
        per = PERIOD_SETS[ps]
        if [piece for piece, _ in missing] == ["m1fd"]:      # (the candidates are known: the reference on them alone)
            v0, e0 = np.zeros((nlay.size, per.size)), np.zeros(nlay.size, dtype=np.int32)
            v0[got["m1"]], e0[got["m1"]] = search(O, nlay[got["m1"]], model[:, :, got["m1"]], per, iwave, 0, threads=threads)
        else:
            v0, e0 = search(O, nlay, model, per, iwave, 0, threads=threads)
        for piece, f in missing:
            if piece == "m1":
                v1, e1 = search(O, nlay, model, per, iwave, 1, threads=threads)
                got[piece] = np.flatnonzero(differs(v1, e1, v0, e0)).astype(np.int32)
            elif piece == "m1fd":   # which of them the guarded restatement (mode 2) does not bring back to the reference
                idx = got["m1"]
                v2, e2 = search(O, nlay[idx], model[:, :, idx], per, iwave, 2, threads=threads)
                got[piece] = differs(v2, e2, v0[idx], e0[idx])
            elif piece == "sec":
                v2, _ = search(O, nlay, model, per, iwave, 0, mode=2, threads=threads)
                got[piece] = np.flatnonzero(close_modes(v0, v2)).astype(np.int32)
            else:
                got[piece] = near_kinds(nlay, model, v0)
            if f:
                np.save(f, got[piece])
    return got


def mine(O, threads, cache, log=print):
    """[(class, near_kind, iwave, period set, chunk, index)] in the order they are kept"""
    cand = {(k, ps, w): [] for k in QUOTA for ps in range(2) for w in WAVES}
    plain = {(ps, w): 0 for ps in range(2) for w in WAVES}   # needs_guard candidates without the label fastm_differs
    need = {k: QUOTA[k] * SPARE[k] for k in QUOTA}

    def open_(k, ps, w):
        if k == "near_bx" and w == 2:
            return False
        return (plain[(ps, w)] if k == "needs_guard" else len(cand[(k, ps, w)])) < need[k]

    for chunk in range(MAX_CHUNKS):
        busy = False
        for ps in range(2):
            for w in WAVES:
                want = [p for p, k in (("m1", "needs_guard"), ("m1fd", "needs_guard"), ("sec", "close_modes")) if open_(k, ps, w)]
                if open_("near_hs", ps, w) or open_("near_bx", ps, w):
                    want.append("near")
                if not want:
                    continue
                busy = True
                t0 = time.time()
                got = scan_chunk(O, chunk, ps, w, want, threads, cache)
                for piece, k in (("m1", "needs_guard"), ("sec", "close_modes")):
                    if piece in got:
                        cand[(k, ps, w)] += [(chunk, int(i)) for i in got[piece]]
                if "m1fd" in got:
                    plain[(ps, w)] += int((~got["m1fd"]).sum())
                if "near" in got:
                    if open_("near_hs", ps, w):
                        cand[("near_hs", ps, w)] += [(chunk, int(i)) for i in np.flatnonzero(got["near"] & 1)]
                    if open_("near_bx", ps, w):
                        cand[("near_bx", ps, w)] += [(chunk, int(i)) for i in np.flatnonzero(got["near"] & 2)]
                log("chunk %d set %d wave %d %s: %.0f s; candidates %s, needs_guard without fastm_differs %d" % (
                    chunk, ps, w, want, time.time() - t0, {k: len(cand[(k, ps, w)]) for k in QUOTA}, plain[(ps, w)]))
        if not busy:
            break
    else:
        raise SystemExit("classes not full after %d chunks: %s" % (MAX_CHUNKS, {k: len(v) for k, v in cand.items()}))
    picks = []
    for ps in range(2):
        picks += [("control", 0, 0, ps, 0, ps * NCONTROL + i) for i in range(NCONTROL)]
    picks.append(("water", 0, 0, 0, 0, 2 * NCONTROL))
    for k, cls, kind in (("needs_guard", "needs_guard", 0), ("close_modes", "close_modes", 0), ("near_hs", "near_halfspace", 0), ("near_bx", "near_halfspace", 1)):
        for ps in range(2):
            for w in WAVES:
                picks += [(cls, kind, w, ps, c, i, QUOTA[k]) for c, i in cand[(k, ps, w)]]
    picks += [("unexplained", 0, w, 1, c, i, len(UNEXPLAINED)) for c, i, w, _, _, _ in UNEXPLAINED]
    return picks


def assemble(O, picks, threads, log=print):
    """the file's arrays from the candidates: both wave types' mode 0 and mode 2 at the candidate's period set, the fastm_differs
    cap, no model twice, every class cut at its quota"""
    chunks = {}
    nl, mods = [], []
    for p in picks:
        c, i = p[4], p[5]
        if c not in chunks:
            chunks[c] = draw(c)
        nlay, model = chunks[c]
        m = model[:, :, i].copy()
        if p[0] == "water":
            m[2, 0], m[1, 0] = 0.0, 1.5
        nl.append(nlay[i])
        mods.append(m)
    nl = np.array(nl, dtype=np.int32)
    mods = np.ascontiguousarray(np.stack(mods, axis=2))                 # [4, L, n]
    pset = np.array([p[3] for p in picks])
    n = len(picks)
    vel = np.zeros((2, n, 2, KMAX))
    err = np.zeros((2, n, 2), dtype=np.int32)
    for ps in range(2):
        sel = np.flatnonzero(pset == ps)
        K = PERIOD_SETS[ps].size
        for iw, w in enumerate(WAVES):
            for j, smode in enumerate((0, 2)):
                v, e = search(O, nl[sel], mods[:, :, sel], PERIOD_SETS[ps], w, smode, threads=threads)
                vel[j, sel, iw, :K], err[j, sel, iw] = v, e
    assert np.array_equal(vel, vel.astype(np.float32).astype(np.float64)), "the reference returns binary32 values"
    fd = np.stack([differs(vel[1, :, iw], err[1, :, iw], vel[0, :, iw], err[0, :, iw]) for iw in range(2)], axis=1)
    total = 2 * NCONTROL + 1 + 4 * QUOTA["needs_guard"] + 4 * QUOTA["close_modes"] + 4 * QUOTA["near_hs"] + 2 * QUOTA["near_bx"]
    cap = int(FASTM_CAP * total)
    keep, seen, count, nfd, slotfd = [], set(), {}, 0, {}
    for j, p in enumerate(picks):
        key = (p[4], p[5])
        slot = (p[0], p[1], p[2], p[3])
        if len(p) > 6 and (key in seen or count.get(slot, 0) >= p[6]):
            continue
        if fd[j].any() and p[0] != "unexplained":
            if nfd >= cap or slotfd.get(slot, 0) >= FASTM_PER_SLOT:
                continue
            nfd += 1
            slotfd[slot] = slotfd.get(slot, 0) + 1
        seen.add(key)
        count[slot] = count.get(slot, 0) + 1
        keep.append(j)
    short = [(p[:4], count.get(p[:4], 0)) for p in picks if len(p) > 6 and p[0] != "unexplained" and count.get(p[:4], 0) < p[6]]
    assert not short, sorted(set(short))
    keep = np.array(keep)
    log("kept %d of %d candidates, fastm_differs on %d outside class unexplained (cap %d)" % (keep.size, n, nfd, cap))
    d = {"classes": np.array(CLASSES), "waves": np.array(WAVES, dtype=np.int8), "periods_0": PERIOD_SETS[0], "periods_1": PERIOD_SETS[1],
         "cls": np.array([CLASSES.index(picks[j][0]) for j in keep], dtype=np.int8),
         "near_kind": np.array([picks[j][1] for j in keep], dtype=np.int8),
         "sel_wave": np.array([picks[j][2] for j in keep], dtype=np.int8),
         "pset": pset[keep].astype(np.int8),
         "src": np.array([[picks[j][4], picks[j][5]] for j in keep], dtype=np.int32),
         "nlay": nl[keep], "model": np.ascontiguousarray(mods[:, :, keep]),
         "vel0": vel[0, keep].astype(np.float32), "err0": err[0, keep].astype(np.int8),
         "vel2": vel[1, keep].astype(np.float32), "err2": err[1, keep].astype(np.int8),
         "fastm_differs": fd[keep]}
    return d


def apply_exceptions(O, d, log=print):
    """move the listed models to known_exception / unexplained and keep probe_cell's numbers beside them"""
    ex_row, ex_wave, ex_k, ex_probe = [], [], [], []
    for chunk, index, iwave, k, cls, vengine in EXCEPTIONS + UNEXPLAINED:
        row = np.flatnonzero((d["src"][:, 0] == chunk) & (d["src"][:, 1] == index) & (d["cls"] != CLASSES.index("water")))
        assert row.size == 1, (chunk, index)
        row = int(row[0])
        d["cls"][row] = CLASSES.index(cls)
        per = PERIOD_SETS[d["pset"][row]]
        ref = float(d["vel0"][row, WAVES.index(iwave), k])
        pr, ch, gd, j, apart = probe_pair(O, d["nlay"][row], d["model"][:, :, row], per, k, iwave, ref, vengine)
        log("exception %s: reference %.9g, engine %.9g; sign changes %s, nearest to a grid point %.3g c, its neighbour %.3g km/s away" % (
            (chunk, index, iwave, k, cls), ref, vengine, ch.tolist(), gd[j], apart))
        ex_row.append(row); ex_wave.append(iwave); ex_k.append(k)
        ex_probe.append([ref, vengine, pr["grid_start"], pr["cell"], gd[j], apart] + list(ch[:6]) + [0.0] * (6 - len(ch[:6])))
    d["ex_row"] = np.array(ex_row, dtype=np.int32)
    d["ex_wave"] = np.array(ex_wave, dtype=np.int8)
    d["ex_period"] = np.array(ex_k, dtype=np.int32)
    d["ex_probe"] = np.array(ex_probe, dtype=np.float64).reshape(len(ex_row), 12)
    d["ex_kind"] = np.array([exception_like(p[4], p[5]) for p in ex_probe], dtype=np.int8)
    return d


def probe_pair(O, nlay, model, periods, k, iwave, ref, vengine, step=1e-7):
    """probe_cell where a pair of sign changes must sit if the reference (root ref) and the default path (velocity vengine) ended
    on different roots at period k: at the lower of the two -- the search that saw no sign change there walked on to the other.
    Returns (probe, sign changes, their distances from the nearest grid point relative to c, index of the nearest, distance of
    its neighbouring sign change in km/s)."""
    pr = probe_cell(dict(nlay=nlay, model=model, periods=periods), periods[k], iwave, oracle=O, step=step, at=min(ref, vengine))
    ch, gd = pr["changes"], pr["grid_distance"]
    if ch.size == 0:          # (no sign change in the three cells: the other search ended further away than they reach)
        ch, gd = np.zeros(1), np.array([np.inf])
    j = int(np.argmin(gd))
    apart = float(np.min(np.abs(np.delete(ch, j) - ch[j]))) if ch.size > 1 else np.inf
    return pr, ch, gd, j, apart


def exception_like(grid_distance, apart):
    """the documented exception by the probe's numbers: a sign change within 1e-6 c of a grid point, its neighbour less than a step away"""
    return bool(grid_distance <= 1e-6 and apart < DC)


def _start_velocity(O, a32, b32):
    """the reference's first start value: 0.9 x 0.95 x the Rayleigh velocity of a half-space of the slowest layer (binary32)"""
    j = int(np.argmin(np.where(b32 > 0.01, b32, a32)))
    c = a32[j] if b32[j] <= 0.01 else np.float32(O.gtsolh(a32[j], b32[j]))
    return float(np.float32(0.90) * (np.float32(0.95) * np.float32(c)))


def probe_cell(model, period, wave, oracle=None, step=1e-7, at=None):
    """The reference's secular function (oracle.dltar) on a fine grid -- step <= 1e-7 c -- over three cells of the reference's scan
    at `period`: the cell that holds the reference's root of that period and its two neighbours.  The reference's grid starts at
    c(k-1) - 1.5 dc (dc = 0.005; the first period's at the start velocity) and is walked by repeated addition, as here.

    model: dict(nlay, model [4, L] = h, vp, vs, rho, periods: the period set the search runs over, which must hold `period`);
    wave: 1 Love, 2 Rayleigh; at: a velocity whose cell is the middle one instead of the root's (where another search ended).
    Returns dict(root, grid_start, cell (index of the middle cell; negative: below the start value), edges [4], root_to_grid
    (distance of the root from the nearer edge of its cell, relative to the root), changes (velocities at which the sign changes:
    midpoints of fine-grid steps), grid_distance (of every change from the nearest of the four grid points, relative),
    changes_in_root_cell (in the middle cell), values_at_edges [4]); None where the reference has no root at that period."""
    if oracle is None:
        from oracle import oracle as oracle_
        oracle = oracle_
    O = oracle
    n = int(model["nlay"])
    m = np.asarray(model["model"], dtype=np.float64)[:, :n]
    per = np.asarray(model["periods"], dtype=np.float64)
    k = int(np.flatnonzero(per == period)[0])
    O.set_swd_search(0)
    v, e, _ = O.swd_batch(np.array([n], dtype=np.int32), m[0][None], m[1][None], m[2][None], m[3][None], per, wave, 0)
    if v[0, k] == 0:
        return None
    d, a, b, rho = (x.astype(np.float32) for x in m)
    # (the search carries its roots as binary64; what it returns is their binary32 value: the grid is placed to 1e-7 c, which
    #  is the fine grid's own step)
    root = float(v[0, k])
    start = _start_velocity(O, a, b) if k == 0 else float(v[0, k - 1]) - 1.5 * DC
    cell = int(np.floor(((root if at is None else float(at)) - start) / DC))
    lo = start
    for _ in range(abs(cell - 1)):
        lo = lo + DC if cell - 1 > 0 else lo - DC
    edges = [lo]
    for _ in range(3):
        edges.append(edges[-1] + DC)
    omega = 2.0 * 3.141592653589793 / float(period)
    npts = int(np.ceil((edges[3] - edges[0]) / (step * edges[0]))) + 1
    cs = np.linspace(edges[0], edges[3], npts)
    f = np.array([O.dltar(omega / c, omega, 1 if wave == 1 else 2, d, a, b, rho) for c in cs])
    neg = np.signbit(f)
    at = np.flatnonzero(neg[1:] != neg[:-1])
    changes = 0.5 * (cs[at] + cs[at + 1])
    inside = int(((changes > edges[1]) & (changes < edges[2])).sum())
    fe = [O.dltar(omega / c, omega, 1 if wave == 1 else 2, d, a, b, rho) for c in edges]
    gd = np.array([np.min(np.abs(c - np.array(edges))) / c for c in changes])
    return dict(root=root, grid_start=start, cell=cell, edges=np.array(edges), root_to_grid=min(abs(root - edges[1]), abs(root - edges[2])) / root,
                changes=changes, grid_distance=gd, changes_in_root_cell=inside, values_at_edges=np.array(fe))


def save_npz(path, d):
    """np.savez_compressed with fixed time stamps and a fixed order: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(d):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(d[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue(), compresslevel=9)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--threads", type=int, default=8, help="oracle threads (the result does not depend on them)")
    ap.add_argument("--cache", default=None, help="directory for the chunks' candidate lists (a rerun then only assembles)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "swd_hard_golden.npz"))
    a = ap.parse_args()
    from oracle import oracle as O
    O.lib()
    if a.cache:
        os.makedirs(a.cache, exist_ok=True)
    t0, c0 = time.time(), time.process_time()
    picks = mine(O, a.threads, a.cache)
    d = apply_exceptions(O, assemble(O, picks, a.threads))
    save_npz(a.out, d)
    size = os.path.getsize(a.out)
    print("%s: %d models, %d bytes; %.0f s wall, %.0f s CPU" % (a.out, d["nlay"].size, size, time.time() - t0, time.process_time() - c0))
    for c, name in enumerate(CLASSES):
        for iw, w in enumerate((0,) + WAVES):
            nn = int(((d["cls"] == c) & (d["sel_wave"] == w)).sum())
            if nn:
                print("  %-16s wave %d: %4d  (sets %s, fastm_differs %d)" % (name, w, nn, np.bincount(d["pset"][(d["cls"] == c) & (d["sel_wave"] == w)], minlength=2).tolist(),
                                                                           int(d["fastm_differs"][(d["cls"] == c) & (d["sel_wave"] == w)].any(axis=1).sum())))
    assert size < 1000000, "the fixture must stay under 1 MB: drop control models"


if __name__ == "__main__":
    main()
