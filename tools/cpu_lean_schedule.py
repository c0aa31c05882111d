#!/usr/bin/env python3
"""A schedule model of the trial-per-lane dispersion launch (swd_lean.hip) on the CPU: what an ORDER of the models is worth.
Dev tool; tests/test_lean_schedule_model.py and tools/gpu_lean_schedule.py import its functions.

  * counted_rounds: per model and target, the rounds the 16-lane search takes, from the oracle's phase velocities (search mode 2)
    with the kernel's window rule: the first period scans from cm (16 grid points a round), every later period's first 14 grid points
    ride along with the previous period's cluster (no round of their own), further ones cost a round per 16, and every period ends
    with one round of clustered trials.  (Not counted: a cluster that misses its root, 0.1 % / 1 % of the periods, and the guard's probes.)
  * the order: the blocked bucket sort of pair_order_blocked_kernel (swd_kernel.hip) for a key per target, four models a
    wavefront, the wavefront's rounds = the most of its models'.
  * the SIMDs: wavefront positions that share a SIMD (`placement`), the Love group a position takes (`love_map`), and the SIMD's
    end: both wavefronts advance at the paired cost per round (22.6 / 17.0 thousand cycles, measured at equal priority: docs/HISTORY.md round 5) until the shorter one ends, the
    other goes on alone at `solo` times its paired cost.  solo = 0.5 is "the end follows the sum of the two"; solo = 1 is "two
    wavefronts do not slow each other down" (then the launch is as long as its longest Rayleigh wavefront, whatever the order).

    python tools/cpu_lean_schedule.py [out.txt]        (the table of profiles/lean_schedule_model.txt)"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

KCYC_R, KCYC_L = 22.6, 17.0      # paired cost of a round at equal priority, thousand cycles (docs/HISTORY.md round 5)
BLOCKS, BUCKETS, MPW = 8, 128, 4  # PAIR_BLOCKS, BLOCK_BUCKETS (swd_kernel.hip); models per wavefront at 16 lanes a model
f32 = np.float32
DC = float(f32(0.005))


def start_values(nlay, vp, vs):
    """cm[B]: the first period's start value, 0.9 x 0.95 x the Rayleigh velocity of the slowest layer (binary32)"""
    from oracle import oracle as O
    cm = np.zeros(nlay.size)
    for b in range(nlay.size):
        n = int(nlay[b])
        j = int(np.argmin(np.where(vs[:n, b] > 0.01, vs[:n, b], vp[:n, b])))
        c = f32(vp[j, b]) if vs[j, b] <= 0.01 else f32(O.gtsolh(vp[j, b], vs[j, b]))
        cm[b] = float(f32(0.90) * (f32(0.95) * c))
    return cm


def love_skip_rounds(nlay, h, vp, vs, rho, periods, lanes=16):
    """m[B]: the whole rounds of the first period's Love scan that the kernel does not run -- all their grid points lie below the
    model's slowest S velocity vmin, where the Love function has no sign change (swd_lean.hip; restated and held against the
    reference's function in tests/test_love_scan_certificate.py).  The rounds rebase the grid, b_1 = cm + (lanes - 1) dc,
    b_j+1 = b_j + lanes dc (n dc is exact in binary64: the kernel's fused operation); m is the largest count with
    b_m + 2 dc <= vmin - dc, and 0 where the model alone does not bound the skipped values away from the guard's rules."""
    cm, om, m = start_values(nlay, vp, vs), 2.0 * np.pi / float(periods[0]), np.zeros(nlay.size, np.int64)
    for i in range(nlay.size):
        n = int(nlay[i])
        if n < 2:
            continue
        b, r, d = [x[:n, i].astype(f32).astype(float) for x in (vs, rho, h)]
        vmin, mumin, dmax = b.min(), (r * (b * b)).min(), d[:n - 1].max()
        if not (om > 0.0 and dmax * om <= 4.5e4 * cm[i] and (mumin * mumin) * ((om * om) * DC) >= 1.0e-18 * (vmin * vmin * vmin)):
            continue
        bm = cm[i]
        while True:
            bn = (lanes - 1 if m[i] == 0 else lanes) * DC + bm
            if not (2.0 * DC + bn <= vmin - DC):
                break
            bm, m[i] = bn, m[i] + 1
    return m


def counted_rounds(nlay, h, vp, vs, rho, periods, iwave, lanes=16, cluster=2, love_skip=False):
    """rounds[B] (0 for a model whose search fails), steps[B, K]: grid steps from every period's start value to its sign change.
    love_skip: a Love target's rounds without those of love_skip_rounds, as the kernel runs them (off by default: the figures of
    profiles/lean_schedule_model.txt and the golden fixture of tests/test_lean_schedule_model.py count every round of the scan)"""
    from oracle import oracle as O
    with O.swd_search(2):
        vel, err, _ = O.swd_batch(nlay, h.T, vp.T, vs.T, rho.T, periods, iwave, 0, mode=1)
    cm = start_values(nlay, vp, vs)
    ride = lanes - cluster
    steps = np.zeros_like(vel)
    steps[:, 0] = np.ceil((vel[:, 0] - cm) / DC)
    steps[:, 1:] = np.ceil((vel[:, 1:] - (vel[:, :-1] - 1.5 * DC)) / DC)
    rounds = rounds_from_steps(steps, lanes, ride)
    if love_skip and iwave == 1:
        rounds = rounds - love_skip_rounds(nlay, h, vp, vs, rho, periods, lanes)
    return rounds * (err == 0), steps


def rounds_from_steps(steps, lanes=16, ride=14):
    """the kernel's window rule (see above); a downward walk (steps <= 0) stays inside the window that rode along"""
    first = 1 + np.where(steps[:, 0] <= lanes - 1, 1, 1 + np.ceil((steps[:, 0] - (lanes - 1)) / lanes))
    later = 1 + np.where(steps[:, 1:] <= ride - 1, 0, np.ceil((steps[:, 1:] - (ride - 1)) / lanes))
    return (first + later.sum(1)).astype(np.int64)


def key_range(nlay, h, vs):
    """the parent's key, both targets: range of the S velocities (pair_cost before this tool)"""
    L = vs.shape[0]
    live = np.arange(L)[:, None] < nlay[None, :]
    v = vs.astype(f32)
    return (np.where(live, v, -np.inf).max(0) - np.where(live, v, np.inf).min(0)).astype(f32)


def key_walk(nlay, h, vs, periods, alpha=1.0, slowness=True):
    """a key from the walk itself, binary32 throughout (what a lane of the ordering launch can do from the model arrays alone):
    the phase velocity of a period ~ 0.92 x the average of vs (slowness: of 1 / vs) over the depth alpha x period x the previous
    period's estimate; the key is the walk's length in grid steps -- first period from cm ~ 0.855 x 0.92 x the slowest layer, every
    later one from 1.5 steps below its predecessor.  Returns (steps[B], rounds[B]): the sum of the steps, and the steps put through
    the kernel's window rule."""
    L, B = vs.shape
    v = vs.astype(f32)
    hh = h.astype(f32)
    lay = np.arange(L)[:, None]
    live = lay < nlay[None, :]
    top = (np.cumsum(hh, 0, dtype=f32) - hh).astype(f32)
    thick = np.where(lay < nlay[None, :] - 1, hh, f32(1e9)).astype(f32)  # (the half-space: everything below)
    w0 = np.where(live, f32(1) / np.maximum(v, f32(0.1)), f32(0)) if slowness else np.where(live, v, f32(0))
    cm = f32(0.855 * 0.92) * np.where(live, v, f32(1e9)).min(0)
    cp = f32(0.92) * v[0]
    c = np.zeros((B, len(periods)), f32)
    for k, t in enumerate(periods):
        z = f32(alpha) * f32(t) * cp
        w = np.clip(z[None, :] - top, f32(0), thick) * live
        avg = w.sum(0) / (w * w0).sum(0) if slowness else (w * w0).sum(0) / w.sum(0)
        cp = (f32(0.92) * avg).astype(f32)
        c[:, k] = cp
    steps = np.zeros_like(c)
    steps[:, 0] = np.ceil((c[:, 0] - cm) / f32(DC))
    steps[:, 1:] = np.ceil((c[:, 1:] - c[:, :-1]) / f32(DC) + f32(1.5))
    return np.maximum(steps, 0).sum(1).astype(f32), rounds_from_steps(steps).astype(f32)


def block_sort(key, blocks=BLOCKS, buckets=BUCKETS):
    """per block: its models (batch indices), longest first: the bucket sort of pair_order_blocked_kernel (inside a bucket: by index)"""
    per = key.size // blocks
    out = []
    for x in range(blocks):
        c = key[x * per:(x + 1) * per].astype(f32)
        cmin, cmax = c.min(), c.max()
        scale = f32(buckets - 1) / (cmax - cmin) if cmax > cmin else f32(0)
        k = np.clip(((cmax - c) * scale).astype(np.int32), 0, buckets - 1)
        out.append(x * per + np.argsort(k, kind="stable"))
    return out


def wave_rounds(sorted_blocks, rounds, mpw=MPW):
    """[block][group]: the most rounds among a group's models"""
    return [rounds[s].reshape(-1, mpw).max(1) for s in sorted_blocks]


def placement_pairs(Q, rule):
    """(Rayleigh position, Love position) of the SIMDs of one XCD; a position is the target's q-th wavefront on that XCD.
    "same": position q of both targets.  "rotate": the dispatcher's rule of build_slot_ranks (engine_swd.hip) carried over to
    workgroups of four -- workgroup i holds R 2i, L 2i, R 2i + 1, L 2i + 1, the CU's second workgroup is i + Q / 4 and sits one SIMD on."""
    if rule == "same":
        return [(q, q) for q in range(Q)]
    h = Q // 4
    pr = []
    for i in range(h):
        pr += [(2 * i, 2 * (i + h) + 1), (2 * (i + h), 2 * i), (2 * i + 1, 2 * (i + h)), (2 * (i + h) + 1, 2 * i + 1)]
    return pr


def simd_ends(wR, wL, pairs, love_map, solo=0.5):
    """end of every SIMD, thousand cycles.  love_map(position, Q) -> the Love group that position takes (parent: Q - 1 - position)"""
    ends = []
    for x in range(len(wR)):
        Q = wR[x].size
        for q, ql in pairs(Q):
            a, b = KCYC_R * wR[x][q], KCYC_L * wL[x][love_map(ql, Q)]
            ends.append(pair_end(a, b, solo))
    return np.array(ends)


def pair_end(a, b, solo):
    """two wavefronts of paired lengths a, b on a SIMD: paired until the shorter ends, then the rest of the longer at `solo`
    of its paired cost (solo = 0.5: (a + b) / 2, the sum rule; solo = 1: max(a, b))"""
    lo, hi = (a, b) if a < b else (b, a)
    return lo + (hi - lo) * solo


def lane_use(w, rounds, mpw=MPW):
    """model-rounds over wavefront-rounds x models: the share of the lanes whose model is still searching"""
    return float(rounds.sum()) / float(sum(x.sum() for x in w) * mpw)


def love_group(p, Q, H=0):
    """the Love group (rank, longest first) that Love position p of an XCD takes: swd_lean_kernel's opposite order.  H = 0 (not a
    launch of two workgroups per CU): Q - 1 - p.  H = Q / 2 positions per pass of workgroups: position p < H shares its SIMD with
    Rayleigh position p + H, p >= H with (p - H) ^ 1, and takes the opposite of that rank."""
    if 2 * H != Q:
        return Q - 1 - p
    return H - 1 - p if p < H else Q - 1 - ((p - H) ^ 1)


def spearman(a, b):
    ra, rb = np.argsort(np.argsort(a, kind="stable")), np.argsort(np.argsort(b, kind="stable"))
    return float(np.corrcoef(ra, rb)[0, 1])


def table(out):
    from bayhunter_amd.synth import synth_models, prior_models, SWD_PERIODS, SEED
    rs = np.random.RandomState(SEED)  # bench.py's build_workload, rank 0: the four batches of the pool
    P = lambda *a: print(*a, file=out, flush=True)
    P("Schedule model of the trial-per-lane launch, c2 (4096 models, 10 layers, Rayleigh + Love, 30 periods; 16 lanes a model):")
    P("longest SIMD over mean SIMD.  placement: which positions share a SIMD (rotate = what the per-wavefront records show);")
    P("solo: cost of a round once the partner has left, as a share of the paired cost (0.5 = the end follows the sum; the records give 0.65)")
    for ib in range(4):
        nlay, h, vp, vs, rho = synth_models(rs, 4096, 10, lvz_frac=0.1)
        RR, _ = counted_rounds(nlay, h, vp, vs, rho, SWD_PERIODS, 2)
        RL, _ = counted_rounds(nlay, h, vp, vs, rho, SWD_PERIODS, 1)
        rng = key_range(nlay, h, vs)
        steps, rnds = key_walk(nlay, h, vs, SWD_PERIODS)
        P("batch %d: counted rounds per model R mean %.1f max %d, L mean %.1f max %d" % (ib, RR.mean(), RR.max(), RL.mean(), RL.max()))
        P("  rank correlation with the counted rounds (R / L): range of vs %.2f / %.2f; predicted walk, steps %.2f / %.2f; predicted walk, rounds %.2f / %.2f"
          % (spearman(rng, RR), spearman(rng, RL), spearman(steps, RR), spearman(steps, RL), spearman(rnds, RR), spearman(rnds, RL)))
        for name, kR, kL in (("range of vs (the key in use)", rng, rng), ("predicted walk, steps", steps, steps),
                             ("counted rounds (no launch can have them)", RR.astype(f32), RL.astype(f32))):
            sR, sL = block_sort(kR), block_sort(kL)
            wR, wL = wave_rounds(sR, RR), wave_rounds(sL, RL)
            P("  key: %-42s wavefront rounds R mean %.1f max %d, L mean %.1f max %d; lanes in use R %.3f L %.3f"
              % (name, np.concatenate(wR).mean(), np.concatenate(wR).max(), np.concatenate(wL).mean(), np.concatenate(wL).max(), lane_use(wR, RR), lane_use(wL, RL)))
            for place in ("same", "rotate"):
                for solo in (0.5, 0.65):
                    row = []
                    for H in (0, 64):
                        e = simd_ends(wR, wL, lambda Q: placement_pairs(Q, place), lambda p, Q: love_group(p, Q, H), solo)
                        row.append((e.max() / e.mean(), e.max(), e.mean()))
                    P("      placement %-6s solo %.2f: opposite order %.3f (longest %.0f, mean %.0f kcycles) | pass-aware opposite order %.3f (longest %.0f)"
                      % (place, solo, row[0][0], row[0][1], row[0][2], row[1][0], row[1][1]))
    P("prior-like batches (2 .. 20 layers, velocities in any order): mixed depths are ordered by depth, no key acts; counted rounds for the record")
    for ib in range(2):
        nlay, h, vp, vs, rho = prior_models(rs, 4096, 20)
        RR, _ = counted_rounds(nlay, h, vp, vs, rho, SWD_PERIODS, 2)
        RL, _ = counted_rounds(nlay, h, vp, vs, rho, SWD_PERIODS, 1)
        ok = (RR > 0) & (RL > 0)
        rng = key_range(nlay, h, vs)
        steps, _ = key_walk(nlay, h, vs, SWD_PERIODS)
        P("  batch %d: searches that fail R %d L %d; of the others: rounds R mean %.1f max %d, L mean %.1f max %d; rank correlation range %.2f / %.2f, walk %.2f / %.2f, layers %.2f / %.2f"
          % (ib, (RR == 0).sum(), (RL == 0).sum(), RR[ok].mean(), RR[ok].max(), RL[ok].mean(), RL[ok].max(), spearman(rng[ok], RR[ok]), spearman(rng[ok], RL[ok]),
             spearman(steps[ok], RR[ok]), spearman(steps[ok], RL[ok]), spearman(nlay[ok], RR[ok]), spearman(nlay[ok], RL[ok])))


if __name__ == "__main__":
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            table(f)
    else:
        table(sys.stdout)
