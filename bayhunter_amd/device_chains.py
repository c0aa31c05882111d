"""Device-resident chains: thousands of rj-McMC chains advanced in lock-step with no host work
per chain.

One iteration = three enqueues on the engine's stream (include/bh_engine.h):
    bh_chain_propose  ->  bh_evaluate_batch (device pointers)  ->  bh_chain_accept
so the per-chain Python of the reference's sampler (src/SingleChain.py:511-589 `iterate`, and the
per-chain loops of `bayhunter_amd.chains.ChainBatch`) disappears from the loop; the host only
counts iterations and takes thinned snapshots of the chain states.

Few chains (BASELINE configs[3]: 8 per GPU) leave the GPU idle: one evaluation launch costs ~1.5 ms
whether it holds 8 or 500 models (the length of ONE model's dispersion root search).  `spec_depth` = d
advances every chain by d iterations per launch instead: the proposals of both outcomes of each of the
next d accept/reject decisions are written down first (bh_chain_propose_window: a binary tree of
2^d - 1 proposals per chain; the draws are a pure function of (chain, iteration)), all of them are
evaluated in ONE bh_evaluate_batch, and bh_chain_accept_window walks the realised path -- the
trajectory of the sequential walk, bit for bit.  Windows end where something outside a chain's own
state changes: proposal-width adaptation (every 1000th iteration), snapshots, temperature exchanges.

Random numbers are counter-based (Philox4x32-10) on the device, so a run is reproducible from
`seed` but is NOT the reference's Mersenne-Twister trajectory: `ChainBatch` is the draw-for-draw
replay of the reference, this class is the throughput mode.  The proposal / validity / acceptance
arithmetic is the same.  It is tested twice: kernel by kernel against tests/chain_ref.py, a numpy
restatement of the reference's step that imports nothing of this package (tests/test_gpu_chain_kernels.py),
and as whole trajectories against `ChainBatch`, the replay, with the same injected draws
(tests/test_gpu_device_chains.py).

The initial state (initial models, noise, covariance-law selection, first likelihood) is produced by
`ChainBatch` exactly as the reference does (SingleChain.py:71-205) and uploaded once.

Storage: the reference keeps every accepted model with its iteration stamp and, when saving,
repeats each by its dwell time and thins to `maxmodels` rows (SingleChain.py:591-690) -- i.e. it
keeps the chain's current model at every `thinning`-th iteration.  Here that sampling is done on
the fly: every `thinning`-th iteration the current state of all chains is copied out, which is the
same estimator without storing what would be thinned away.  (One difference: the reference's
main-phase file starts with the first model ACCEPTED at iteration >= 0; here the main phase starts
with the model that is current at iteration 0.)

record="host" takes those snapshots on the host: run() ends every window at a snapshot iteration, waits for the GPU and copies the
state out -- with thinning 1 (the reference's defaults: maxmodels 50000 for 2048 iterations) every launch is one iteration and
ends in a synchronisation.  record="device" leaves them to the accept kernel, which knows the chain's state before every
iteration of its window (include/bh_engine_chain_record.h): the rows go into a store on the GPU, windows are cut at
adaptations and exchanges only and nothing waits; samples() / save() read the store once and return the same arrays, bit for bit.
"""
import ctypes as C
import os
import os.path as op
from collections import namedtuple

import numpy as np

from .chains import ChainBatch, DEFAULT_INITPARAMS, DEFAULT_PRIORS, _is_fixed
from .engine import BH_CHAIN_MAXDEPTH, BH_CHAIN_MAXLAYERS, ChainConfig, ChainPrior, ChainState, EngineError
from .device_chains_store import ChainStore
from .Targets import JointTarget
from .sites import SiteTargets, gather_slots, scatter_slots, window_site_map


def auto_spec_depth(nchains, budget=None):
    """Speculation depth for `nchains` chains on one GPU: the deepest tree whose nodes (chains x (2^d - 1)
    evaluations per launch) stay within `budget` evaluations -- below ~1000 models a launch of the dispersion kernel
    costs about what 8 models cost (docs/HISTORY.md 3.1: 1.5 ms at B <= 512, 2.0 ms at 1024, 3.0 ms at 2048), so d
    iterations per launch are nearly free; beyond it the launch time grows faster than the depth.
    BH_SPEC_BUDGET overrides the budget (0 = no speculation)."""
    if budget is None:
        budget = int(os.environ.get("BH_SPEC_BUDGET", "1024"))
    d = 1
    while d < BH_CHAIN_MAXDEPTH and nchains * ((1 << (d + 1)) - 1) <= budget:
        d += 1
    return d


def snapshot_count(lo, hi, thinning):
    """The snapshots due in [lo, hi): the iterations i with i % thinning == 0 (Python's non-negative residue: i is negative
    during the burn-in) -- run()'s rule."""
    lo, hi, thinning = int(lo), int(hi), int(thinning)
    if thinning < 1:
        raise ValueError("thinning must be >= 1")
    if hi <= lo:
        return 0
    return -((-hi) // thinning) + ((-lo) // thinning)      # ceil(hi / thinning) - ceil(lo / thinning)


def record_rows(iter_burnin, iter_main, thinning):
    """(rows of phase 1, rows of phase 2) a run takes: the snapshots due in [-iter_burnin, 0) and in [0, iter_main)"""
    return snapshot_count(-int(iter_burnin), 0, thinning), snapshot_count(0, int(iter_main), thinning)


def window_entries(engine, table, rec):
    """The propose and the accept entry of one window, by (a table of priors is present, the device record is active):
    (propose method, its extra arguments, accept method, its extra arguments).  table: None, or (records pointer, records,
    prior_of pointer); rec: None, or the ChainRecord of this window."""
    propose = engine.chain_propose_window if table is None else engine.chain_propose_window_priors
    accept = {(False, False): engine.chain_accept_window, (True, False): engine.chain_accept_window_priors,
              (False, True): engine.chain_accept_window_record,
              (True, True): engine.chain_accept_window_priors_record}[table is not None, rec is not None]
    extra = () if table is None else tuple(table)
    return propose, extra, accept, extra + (() if rec is None else (rec,))


RECORD_MODES = ("host", "device")

# DeviceChains(ladder_adapt=): sweeps per adaptation window, gain and decay of the gain (kappa = rate * lag / (n + lag) at the n-th
# adaptation).  The values of the study on the idealised sampler (tests/test_ladder_sweep_ref.py).
LADDER_ADAPT_DEFAULTS = dict(every=20, rate=0.5, lag=50.0)


def ladder_adapt_options(ladder_adapt, betas, ladder, swap_every, dist=None):
    """The merged options of DeviceChains(ladder_adapt=), checked without a GPU: None stays None.  ValueError: an unknown key, `every`
    not an even integer >= 0, rate outside (0, 1), lag <= 0, no betas or swap_every == 0, with every > 0 a ladder whose betas
    are not distinct.  EngineError: a job of more than one rank, BH_PT_HOST_EXCHANGE=1."""
    if ladder_adapt is None:
        return None
    if not isinstance(ladder_adapt, dict):
        raise ValueError("ladder_adapt must be None or a dict with keys of %s" % (sorted(LADDER_ADAPT_DEFAULTS),))
    unknown = sorted(set(ladder_adapt) - set(LADDER_ADAPT_DEFAULTS))
    if unknown:
        raise ValueError("ladder_adapt: unknown key %r (known: %s)" % (unknown[0], sorted(LADDER_ADAPT_DEFAULTS)))
    opt = dict(LADDER_ADAPT_DEFAULTS)
    opt.update(ladder_adapt)
    every = opt["every"]
    if isinstance(every, bool) or not isinstance(every, (int, np.integer)) or every < 0 or every % 2:
        raise ValueError("ladder_adapt['every'] must be an even integer >= 0 (both parities fall into every window), not %r" % (every,))
    opt["every"] = int(every)
    opt["rate"], opt["lag"] = float(opt["rate"]), float(opt["lag"])
    if not 0.0 < opt["rate"] < 1.0:
        raise ValueError("ladder_adapt['rate'] must lie in (0, 1), not %r" % (opt["rate"],))
    if not (opt["lag"] > 0.0 and np.isfinite(opt["lag"])):
        raise ValueError("ladder_adapt['lag'] must be > 0, not %r" % (opt["lag"],))
    if betas is None or int(swap_every) <= 0:
        raise ValueError("ladder_adapt needs a tempered run: betas and swap_every > 0")
    if opt["every"] > 0:
        b = np.asarray(betas, dtype=np.float64).ravel()
        lad = np.zeros(b.size, dtype=np.int64) if ladder is None else np.asarray(ladder, dtype=np.int64).ravel()
        if lad.size != b.size:
            raise ValueError("ladder_adapt: %d betas for %d ladder ids" % (b.size, lad.size))
        for lid in np.unique(lad):
            if np.unique(b[lad == lid]).size != np.count_nonzero(lad == lid):
                raise ValueError("ladder_adapt: the betas of ladder %d are not distinct (an adapted ladder is strictly ordered)" % lid)
    if dist is not None and dist.is_initialized() and dist.get_world_size() > 1:
        raise EngineError("ladder_adapt: ladders are not adapted across ranks (world size %d)" % dist.get_world_size())
    if os.environ.get("BH_PT_HOST_EXCHANGE", "0") == "1":
        raise EngineError("ladder_adapt: the sweep kernel runs on the GPU; BH_PT_HOST_EXCHANGE=1 asks for the host exchange")
    return opt


# initparams the sites of one run must share: the chains advance in lock step (iter_*), are thinned together (maxmodels), share the
# Gauss law's R^-1 (rcond) and are saved below one root (savepath).  Every other key, and every modelpriors key, may differ per site.
SHARED_INITPARAMS = ("iter_burnin", "iter_main", "maxmodels", "rcond", "savepath")
SITE_INITPARAMS = ("propdist", "acceptance", "thickmin", "lvz", "hvz")


def _same(a, b):
    if a is None or b is None:
        return a is b
    return bool(np.array_equal(np.asarray(a), np.asarray(b)))


def site_dicts(initparams, modelpriors, nsites, with_sites):
    """The merged (initparams, modelpriors) of every site and whether any two sites differ in what the sampler reads.
    Each argument is one dict (or None) for all sites or a sequence of `nsites` dicts; every dict is merged over the defaults.
    ValueError: a sequence without SiteTargets, of another length than the sites, or sites that differ in a SHARED_INITPARAMS
    key; EngineError: a site's priors['layers'][1] + 1 beyond BH_CHAIN_MAXLAYERS."""
    def spread(arg, defaults, what):
        if isinstance(arg, (list, tuple)):
            if not with_sites:
                raise ValueError("a sequence of %s dicts needs SiteTargets (one dict per site)" % what)
            if len(arg) != nsites:
                raise ValueError("%d %s dicts for %d sites" % (len(arg), what, nsites))
            given = list(arg)
        else:
            given = [arg] * nsites
        out = []
        for g in given:
            d = dict(defaults)
            d.update(g or {})
            out.append(d)
        return out

    ips = spread(initparams, DEFAULT_INITPARAMS, "initparams")
    prs = spread(modelpriors, DEFAULT_PRIORS, "modelpriors")
    for s in range(1, nsites):
        for key in SHARED_INITPARAMS:
            if not _same(ips[s].get(key), ips[0].get(key)):
                raise ValueError("initparams[%r] of site %d is %r, site 0's %r: the sites of one run share it"
                                 % (key, s, ips[s].get(key), ips[0].get(key)))
    for s, pr in enumerate(prs):
        if int(pr["layers"][1]) + 1 > BH_CHAIN_MAXLAYERS:
            raise EngineError("%spriors['layers'][1] + 1 = %d exceeds BH_CHAIN_MAXLAYERS = %d"
                              % ("site %d: " % s if with_sites else "", int(pr["layers"][1]) + 1, BH_CHAIN_MAXLAYERS))
    differ = any(not _same(prs[s].get(k), prs[0].get(k)) for s in range(1, nsites) for k in set(prs[0]) | set(prs[s])) or \
        any(not _same(ips[s].get(k), ips[0].get(k)) for s in range(1, nsites) for k in SITE_INITPARAMS)
    return ips, prs, differ


def set_station_fields(rec, ip, pr, noisepriors):
    """Fill the station fields of a ChainConfig or a ChainPrior (they carry the same names) from merged initparams `ip`, merged
    priors `pr` and the list of noise priors (corr, sigma per target): a fixed prior as lo == hi, None as -1."""
    rec.layermin, rec.layermax = int(pr["layers"][0]), int(pr["layers"][1])
    (rec.vsmin, rec.vsmax), (rec.zmin, rec.zmax) = pr["vs"], pr["z"]
    rec.thickmin = ip["thickmin"]
    rec.lvz = -1.0 if ip["lvz"] is None else ip["lvz"]
    rec.hvz = -1.0 if ip["hvz"] is None else ip["hvz"]
    if _is_fixed(pr["vpvs"]):
        rec.vpvsmin = rec.vpvsmax = float(pr["vpvs"])
    else:
        rec.vpvsmin, rec.vpvsmax = pr["vpvs"]
    if pr["mantle"] is None:
        rec.mantle_vs, rec.mantle_vpvs = -1.0, 0.0
    else:
        rec.mantle_vs, rec.mantle_vpvs = pr["mantle"]
    rec.acc_lo, rec.acc_hi = ip["acceptance"]
    for i, p in enumerate(noisepriors):
        if _is_fixed(p):
            rec.noise_lo[i] = rec.noise_hi[i] = float(p)
        else:
            rec.noise_lo[i], rec.noise_hi[i] = p
    return rec


ChainPlan = namedtuple("ChainPlan", "record ladder_adapt search arith prior_table nsites site_initparams site_priors present C_site C nt "
                                    "site_ML ML iter_phase1 iter_phase2 iterations thinning depth ld ladder site_map absent")


def plan_chains(targets, nchains, initparams=None, modelpriors=None, betas=None, ladder=None, swap_every=0, dist=None, spec_depth=None,
                search="fast", arith="fast", prior_table=False, record="host", ladder_adapt=None):
    """What DeviceChains(...) settles before it needs a GPU, as a ChainPlan: the checked options (record, ladder_adapt merged by
    `ladder_adapt_options`, search, arith, prior_table = the table of priors is in use), the merged dicts of every site
    (`site_dicts`), the sizes (C_site chains per site, C on this rank, nt targets, a site's row capacity site_ML and the arrays'
    ML, the iteration counts, thinning, the speculation depth and ld = the columns of the proposal arrays), the ladder ids
    (int64 [C], None untempered) and, as numpy arrays, the sites' tables: present (bool [nsites, nt], SiteTargets(missing=True)),
    site_map (`window_site_map`, SiteTargets) and absent (uint8 [C], bit i set: the chain's site lacks slot i), None where they
    do not apply.  `targets` (a SiteTargets, a JointTarget or a list of targets) is read, never registered: no engine is made.
    Raises what the constructor refuses, in its order."""
    if record not in RECORD_MODES:      # (before the targets are looked at)
        raise ValueError("record must be 'host' or 'device', not %r" % (record,))
    adapt = ladder_adapt_options(ladder_adapt, betas, ladder, swap_every, dist)
    sites = targets if isinstance(targets, SiteTargets) else None
    nsites = 1 if sites is None else sites.nsites
    if sites is None:   # (SiteTargets refuses it itself: "a user plugin")
        from .Targets import RayleighEllipticity
        for t in (targets.targets if isinstance(targets, JointTarget) else targets):
            if isinstance(t, RayleighEllipticity) and not t.engine_backed():   # (fused=True: part of the fused call)
                raise EngineError("DeviceChains does not run RayleighEllipticity: the device chains evaluate engine-backed "
                                  "targets in one fused call, and the ellipticity is not part of it yet (ChainBatch runs it)")
    ips, prs, differ = site_dicts(initparams, modelpriors, nsites, sites is not None)
    if prior_table and sites is None:
        raise ValueError("prior_table=True needs SiteTargets")
    if sites is not None and dist is not None:
        raise EngineError("DeviceChains with SiteTargets does not shard: give each process its own sites instead of dist")
    if search not in (None, "reference", "fast", "fast_rayleigh"):
        raise ValueError("search must be None, 'reference', 'fast' or 'fast_rayleigh'")
    if arith not in (None, "exact", "fast"):
        raise ValueError("arith must be None, 'exact' or 'fast'")
    C_site = int(nchains)                             # chains per site (sites: S blocks of them, site after site)
    Cn = C_site * nsites
    nt = targets.ntargets if isinstance(targets, (JointTarget, SiteTargets)) else len(targets)
    site_ML = [int(pr["layers"][1]) + 1 for pr in prs]    # a site's own row capacity; the arrays have the rows of the largest
    iter_phase1, iter_phase2 = int(ips[0]["iter_burnin"]), int(ips[0]["iter_main"])
    thinning = max(1, int(np.ceil(float(iter_phase2) / float(ips[0]["maxmodels"]))))
    depth = auto_spec_depth(Cn) if spec_depth is None else int(spec_depth)
    if not 1 <= depth <= BH_CHAIN_MAXDEPTH:
        raise EngineError("spec_depth must be 1..%d" % BH_CHAIN_MAXDEPTH)
    ld = Cn * ((1 << depth) - 1)                      # columns of the proposal arrays: all nodes of all chains
    lad = None if betas is None else np.asarray(ladder if ladder is not None else np.zeros(Cn), dtype=np.int64)
    if sites is not None and lad is not None:
        of = np.arange(Cn) // C_site
        for lid in np.unique(lad):
            if np.unique(of[lad == lid]).size > 1:
                raise EngineError("tempering ladder %d spans sites: every ladder must lie within one site" % lid)
    present = None if sites is None or not sites.missing else sites.present
    absent = None if present is None else np.repeat(((~present).astype(np.int64) << np.arange(nt)).sum(axis=1).astype(np.uint8), C_site)
    return ChainPlan(record, adapt, search, arith, bool(differ or prior_table), nsites, ips, prs, present, C_site, Cn, nt, site_ML,
                     max(site_ML), iter_phase1, iter_phase2, iter_phase1 + iter_phase2, thinning, depth, ld, lad,
                     None if sites is None else window_site_map(C_site, nsites, ld), absent)


def merge_noisepriors(site_lists, present, nt, table):
    """(noisepriors, site_noisepriors) of a run from every site's own list (ChainBatch.noisepriors: corr, sigma per target the site
    has).  table: (None, one list per site in the slot layout; a slot the site lacks: fixed at 0 -- and masked by `absent`).
    Else (the one list the sites share, None): with every slot everywhere (present None) the sites' lists must be equal, with
    missing slots every slot's pair must agree among the sites that have it.  EngineError: "the sites' noise priors differ"."""
    if table:
        rows = []
        for s, own in enumerate(site_lists):
            have = np.arange(nt) if present is None else np.flatnonzero(present[s])
            row = [0.0] * (2 * nt)
            for j, i in enumerate(have):
                row[2 * i], row[2 * i + 1] = own[2 * j], own[2 * j + 1]
            rows.append(row)
        return None, rows
    if present is None:
        if any(own != site_lists[0] for own in site_lists):
            raise EngineError("the sites' noise priors differ")
        return site_lists[0], None
    shared = [None] * (2 * nt)   # (a site's own list holds its present targets' only)
    for s, own in enumerate(site_lists):
        for j, i in enumerate(np.flatnonzero(present[s])):
            for k in (0, 1):
                if shared[2 * i + k] is None:
                    shared[2 * i + k] = own[2 * j + k]
                elif shared[2 * i + k] != own[2 * j + k]:
                    raise EngineError("the sites' noise priors differ")
    return shared, None


def initial_state_arrays(host_chains, ML, nt, present, C_site):
    """The state the reference-order host chains start with, packed for the device: a dict of n int32 [C], vs and z [ML, C] (a
    chain's layers first, zeros after), noise [2nt, C], misfits [nt + 1, C], like and vpvs [C], propdist [5, C] (float64), chain c
    in column c.  present (SiteTargets(missing=True)): the chains of site c // C_site hold their site's own noise and misfit
    layout, which goes into the slot layout (`scatter_slots`).  Reads currentmodel, currentnoise, currentmisfits,
    currentlikelihood, currentvpvs and propdist of every chain."""
    Cn = len(host_chains)
    a = dict(n=np.zeros(Cn, dtype=np.int32), vs=np.zeros((ML, Cn)), z=np.zeros((ML, Cn)), noise=np.zeros((2 * nt, Cn)),
             misfits=np.zeros((nt + 1, Cn)), like=np.zeros(Cn), vpvs=np.zeros(Cn), propdist=np.zeros((5, Cn)))
    for c, ch in enumerate(host_chains):
        m = np.asarray(ch.currentmodel, dtype=float)
        n = m.size // 2
        a["n"][c] = n
        a["vs"][:n, c], a["z"][:n, c] = m[:n], m[n:]
        if present is None:
            a["noise"][:, c], a["misfits"][:, c] = ch.currentnoise, ch.currentmisfits
        else:   # the site's own layout into the slot layout
            a["noise"][:, c], a["misfits"][:, c] = scatter_slots(present[c // C_site], ch.currentnoise, ch.currentmisfits)
        a["like"][c], a["vpvs"][c] = ch.currentlikelihood, ch.currentvpvs
        a["propdist"][:, c] = ch.propdist
    return a


def _host_rows(snapshots, C, ML, nt):
    """the rows of samples() from the host snapshots of run(): `snapshots` = the dicts _snapshot() keeps of one phase"""
    ns = len(snapshots)
    models = np.full((ns, C, 2 * ML), np.nan, dtype=np.float32)
    j = np.arange(2 * ML)[:, None]                               # position inside a reference row
    for i, r in enumerate(snapshots):
        n = r["n"][None, :].astype(np.int64)                      # [1, C]
        # reference rows hold the n vs values first, then the n depths, then NaN padding
        both = np.vstack((r["vs"], r["z"]))                       # [2*ML, C]: vs rows, then z rows
        src = np.where(j < n, j, ML + (j - n))                    # row of `both` feeding position j
        row = np.take_along_axis(both, np.clip(src, 0, 2 * ML - 1), axis=0)
        models[i] = np.where(j < 2 * n, row, np.nan).T
    out = dict(models=models)
    for k in ("like", "vpvs"):
        out[k + "s" if k == "like" else k] = np.array([r[k] for r in snapshots], dtype=np.float32).reshape(ns, C)
    out["misfits"] = np.array([r["misfits"].T for r in snapshots], dtype=np.float32).reshape(ns, C, nt + 1)
    out["noise"] = np.array([r["noise"].T for r in snapshots], dtype=np.float32).reshape(ns, C, 2 * nt)
    if ns and snapshots[0]["beta"] is not None:
        out["beta"] = np.array([r["beta"] for r in snapshots]).reshape(ns, C)   # cold samples: out["beta"] == 1
    return out


class DeviceChains(ChainStore):
    """`nchains` chains on THIS rank.  Sharded jobs (one process per GPU, `dist` = an initialised
    torch.distributed): `seed` is the JOB's seed, the same on every rank; the chains are numbered globally
    (`chain_offset` = global index of this rank's first chain, default: ranks own consecutive blocks in rank
    order) and every chain's random stream and initial state depend on (seed, global index) only -- N ranks x C
    chains walk exactly the trajectories of one rank with N*C chains.
    betas / ladder / swap_every: parallel tempering (no counterpart in the reference).  `betas[c]` is the
    inverse temperature chain c starts with, `ladder[c]` the id of the temperature ladder it belongs to (ids
    are global across ranks); every `swap_every` iterations neighbouring temperatures of each ladder are
    exchanged (`parallel.tempering_exchange`, decisions drawn from the job seed: identical on every rank;
    chains keep their states and swap betas, so nothing but (logL, beta, ladder) of each chain crosses GPUs).
    Posterior samples are the snapshots of the chains that hold beta = 1 at that time
    (`samples(cold_only=True)`, and what `save()` writes).
    device: CUDA device index; default = the engine's (`JointTarget(..., engine=)`), else 0.
    spec_depth: iterations per evaluation launch (speculative window, 1..7; module docstring).  None = chosen
    from the number of chains so that a launch stays in the latency regime (`auto_spec_depth`); 1 = one
    iteration per launch.  Results do not depend on it.
    search: root refinement of the dispersion search in the chains' evaluation launches (Engine.set_swd_search;
    applied around every launch, the engine's own setting is left as it was).  Default "fast" (the engine's own
    default): fundamental-mode phase velocities within 1.2e-6 relative of the reference's, the reference's failure
    flags (a model the guard fires on -- 2 % of a sampler's Love proposals -- starts again with the reference's
    sequence inside its own wavefront of the window's launch), group velocities the reference's bits -- what the
    chains sample does not change (tests/test_gpu_device_chains.py::test_search_modes_sample_the_same_posterior),
    a window takes 22-27 % less.  "fast_rayleigh": the short refinement for the Rayleigh targets only.
    "reference": the reference's bits throughout (what `ChainBatch`, the replay of recorded reference runs, uses);
    None: whatever the engine is set to.
    arith: arithmetic of those launches where every dispersion target takes the short refinement (Engine.set_swd_arith,
    applied like `search`).  Default "fast" (the engine's own): the windows run the trial-per-lane kernel with 32 trials
    per round whatever their size (Engine.set_swd_trials), so that windows of any depth and shards of any size walk the
    same trajectory; its guarded models (2 % of a sampler's Love proposals) are re-run by a second launch.  "exact": the
    reference's rounding points -- the windows then take the layer-parallel kernel, which restarts a guarded model in
    place.  Measured on MI355X (chain-iterations/s, "fast" / "exact"): 8 chains 7.4e4 / 5.2e4, a 64-chain tempered rung
    2.18e5 / 1.83e5, 512 chains 4.6e5 / 3.9e5.  None: whatever the engine is set to.
    Many stations: `targets` = a SiteTargets of S sites runs `nchains` chains PER SITE in one lock-step launch: chain c of
    site s is chain s*nchains + c (plus chain_offset) and walks exactly the trajectory of a one-site
    DeviceChains(site s, nchains, chain_offset=s*nchains) with the same seed; every model of a window is compared with
    its own site's data (Engine.evaluate_sites_dev).  Tempering ladders must lie within one site; `dist` is refused
    (spread sites over GPUs by giving each process its own sites).  SiteTargets(missing=True): a site's chains walk the
    one-site run over the targets the site HAS -- the noise parameters of a slot it lacks are never proposed (a mask per
    chain goes to the proposal kernels) --, `samples(site=s)` and the saved files hold the noise and misfit columns of
    the site's own targets; `samples()` of all chains is in the slot layout.
    Priors per site: with SiteTargets, `initparams` and `modelpriors` may each be a sequence of one dict per site (each merged
    over the defaults).  Every modelpriors key and the initparams propdist / acceptance / thickmin / lvz / hvz may differ;
    SHARED_INITPARAMS must agree (ValueError).  A site's chains then run under the site's own record of a table
    (include/bh_engine_sites_priors.h) and walk the one-site run made with the site's dicts, bit for bit; the arrays have the
    rows of the largest `layers` maximum, `samples(site=s)`, the saved chain files and <name>_config.pkl the site's own row
    width, priors and initparams.  The sites share every slot's installed noise law (SiteTargets.check) unless the set was
    made with per_site_law=True, which gives every (site, slot) the law its own priors install.  Sites whose merged dicts agree, or one dict, take the calls without a table exactly as before; prior_table=True forces the table
    (for measurements).  `self.priors` / `self.initparams` are site 0's; `self.site_priors` / `self.site_initparams` every
    site's.
    record: "host" (default) -- run() copies the chains' state out at every `thinning`-th iteration, and its windows end
    there; "device" -- the accept kernel writes those rows into a store on the GPU (rows of both phases, allocated here:
    EngineError if it does not fit the free memory), run() cuts no window and waits for nothing, `samples()` and `save()`
    return what they return with "host", bit for bit, and `samples_dev()` hands the rows to the posterior kernels where they
    lie.  A bare `iterate()` loop outside run() records as well, by the same rule, while iiter < iter_main.  Sharded runs
    keep the host gather of `samples()`.
    ladder_adapt: None (default) -- the exchange sweeps are `parallel.DeviceExchange`'s, nothing is counted per pair.  A dict,
    merged over LADDER_ADAPT_DEFAULTS (every = 20, rate = 0.5, lag = 50) -- the sweeps are one kernel each
    (`parallel.KernelExchange`, include/bh_engine_chain_ladder_sweep.h): the same decisions, counted per neighbouring pair of
    rungs (`ladder_swaps()`), and during the burn-in the interior temperatures of every ladder of three or more chains move
    after every `every` sweeps so that the pairs' acceptance rates equalise; a ladder's largest and smallest beta never change.
    `every` = 0 counts and never adapts (the run is then the run without ladder_adapt, bit for bit).  A sweep after a window
    that ends at iiter <= 0 belongs to the burn-in; the temperatures are frozen from the first main-phase iteration on --
    adapting while sampling would break detailed balance, what the burn-in adapts is discarded with it.  ValueError /
    EngineError: `ladder_adapt_options`."""
    TRIALS = 32  # trials per round of the trial-per-lane kernel in every evaluation call of the chains (windows and initial state)

    def __init__(self, targets, nchains, initparams=None, modelpriors=None, seed=0, device=None, inject=False,
                 betas=None, ladder=None, swap_every=0, dist=None, chain_offset=None, spec_depth=None, search="fast", arith="fast",
                 prior_table=False, record="host", ladder_adapt=None):
        p = self.plan = plan_chains(targets, nchains, initparams, modelpriors, betas, ladder, swap_every, dist, spec_depth, search, arith,
                                    prior_table, record, ladder_adapt)  # (every refusal that needs no GPU: before anything touches it)
        self.record, self.ladder_adapt, self.search, self.arith, self.prior_table = p.record, p.ladder_adapt, p.search, p.arith, p.prior_table
        self.sites = targets if isinstance(targets, SiteTargets) else None
        self.nsites, self.site_initparams, self.site_priors, self.present = p.nsites, p.site_initparams, p.site_priors, p.present
        self.C_site, self.C, self.nt, self.site_ML, self.ML = p.C_site, p.C, p.nt, p.site_ML, p.ML
        self.iter_phase1, self.iter_phase2, self.iterations, self.thinning = p.iter_phase1, p.iter_phase2, p.iterations, p.thinning
        self.depth, self.ld, self.ladder = p.depth, p.ld, p.ladder
        import torch
        self.torch = torch
        self.targets = targets if isinstance(targets, (JointTarget, SiteTargets)) else JointTarget(targets)
        if self.targets._engine is None and device is not None:
            from .engine import default_engine
            self.targets._engine = default_engine(int(device))   # kernels and tensors on the same GPU
        self.engine = self.targets.engine
        if device is None:
            device = self.engine.device
        if int(device) != int(self.engine.device):
            raise EngineError("DeviceChains(device=%d) but the targets' engine runs on GPU %d" % (device, self.engine.device))
        self.initparams, self.priors = self.site_initparams[0], self.site_priors[0]
        self.iiter = -self.iter_phase1
        self.swap_every, self.dist, self._nswaps_host, self.sweep, self.seed = int(swap_every), dist, 0, 0, int(seed)
        self.snap_in_run = False                          # run(): windows also end at snapshot iterations
        self.launches, self._hint, self._dev_exchange = 0, 0, None
        from .parallel import chain_layout, chain_seeds, rank_chain_counts
        self.rank_counts = rank_chain_counts(self.C, dist, int(device))       # collective buffers on THIS rank's GPU
        off, tot = chain_layout(self.C, dist, int(device))
        if chain_offset is not None:
            off = int(chain_offset)
        self.chain_offset, self.C_global = off, max(tot, off + self.C)
        self.rank = dist.get_rank() if dist is not None and dist.is_initialized() else 0

        # ---- initial state through the reference-order host code --------------------------------
        # (sites: one ChainBatch per site, on that site's targets, with the seeds of its global chain numbers)
        hosts = [ChainBatch(self.targets if self.sites is None else self.sites.site(s),
                            chain_seeds(seed, off + s * self.C_site, self.C_site), self.site_initparams[s], self.site_priors[s],
                            search=self.search if self.search is not None else self.targets.engine.swd_search(),
                            arith=self.arith if self.arith is not None else self.targets.engine.swd_arith(),
                            trials=self.TRIALS)   # (the windows' count: the initial likelihoods are the windows' bits)
                 for s in range(self.nsites)]
        self.noisepriors, self.site_noisepriors = merge_noisepriors([h.noisepriors for h in hosts], self.present, self.nt, self.prior_table)
        host_chains = [ch for h in hosts for ch in h.chains]
        self.targets._register()  # constant target data + laws (+ the site table) live on the device from here on

        cfg = ChainConfig()
        cfg.nt, cfg.maxlayers = self.nt, self.ML
        cfg.iter_burnin, cfg.iterations = self.iter_phase1, self.iterations
        records = None
        if self.prior_table:    # the station fields of cfg are not read: every chain has its site's record
            records = (ChainPrior * self.nsites)()
            for s in range(self.nsites):
                set_station_fields(records[s], self.site_initparams[s], self.site_priors[s], self.site_noisepriors[s])
        else:
            set_station_fields(cfg, self.initparams, self.priors, self.noisepriors)
        cfg.seed, cfg.chain_offset = int(seed) & (2 ** 64 - 1), off
        self.cfg = cfg

        dev = self.dev = torch.device("cuda", int(device))
        Cn, ML, nt, ld = self.C, self.ML, self.nt, self.ld
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        t = {k: torch.from_numpy(a).to(dev) for k, a in initial_state_arrays(host_chains, ML, nt, self.present, self.C_site).items()}
        t["proposed"], t["accepted"] = torch.zeros((5, Cn), **f64), torch.zeros((5, Cn), **f64)
        t["naccepted"] = torch.zeros(Cn, dtype=torch.int64, device=dev)
        t["beta"] = None if betas is None else torch.as_tensor(np.asarray(betas, dtype=np.float64)).to(dev)
        # (sites) every window column's site; (missing=True) per chain, bit i set: its site lacks slot i -- that noise is not free there
        self.site_map = None if p.site_map is None else torch.from_numpy(p.site_map).to(dev)
        self.absent = None if p.absent is None else torch.from_numpy(p.absent).to(dev)
        # (priors per site) the table of records and, per chain, its site's record
        self.prior_records = self.prior_of = None
        if records is not None:
            self.prior_records = torch.from_numpy(np.frombuffer(records, dtype=np.uint8).copy()).to(dev)
            self.prior_of = torch.from_numpy(np.repeat(np.arange(self.nsites, dtype=np.int32), self.C_site)).to(dev)
        for k in ("pn", "move", "valid", "lay_n"):        # node j of chain c in column j*C + c
            t[k] = torch.zeros(ld, **i32)
        for k in ("pvs", "pz", "lay_h", "lay_vp", "lay_vs", "lay_rho"):
            t[k] = torch.zeros((ML, ld), **f64)
        t["pvpvs"], t["dvs2"] = torch.zeros(ld, **f64), torch.zeros(ld, **f64)
        t["pnoise"] = torch.zeros((ld, 2 * nt), **f64)
        t["inject"] = torch.zeros((self.depth, 6, Cn), **f64) if inject else None
        self.t = t
        # outputs of the evaluate call of the current window
        self.logL = torch.zeros(ld, **f64)
        self.mis = torch.zeros((ld, nt + 1), **f64)
        self.err = torch.zeros(ld, **i32)
        st = ChainState()
        for k in ChainState._fields_:
            v = t[k[0]]
            setattr(st, k[0], None if v is None else v.data_ptr())
        self.state = st
        self.store = self._rec = None
        if self.record == "device":
            self._allocate_store(betas is not None)
        torch.cuda.synchronize(dev)
        self._ext_stream = torch.cuda.ExternalStream(int(self.engine.stream), device=dev)   # the engine's stream, for torch work
        # replica exchange on the device (one rank, or RCCL): the ladder of every chain of the job is static
        if betas is not None and self.swap_every > 0:
            on_gpu = dist is None or not dist.is_initialized() or dist.get_world_size() == 1 or dist.get_backend() == "nccl"
            if self.ladder_adapt is not None:       # (one rank: ladder_adapt_options)
                from .parallel import KernelExchange
                with torch.cuda.stream(self._ext_stream):
                    self._dev_exchange = KernelExchange(self.engine, self.ladder, self.seed, dev, rate=self.ladder_adapt["rate"],
                                                        lag=self.ladder_adapt["lag"])
                self._betas0 = np.asarray(betas, dtype=np.float64).copy()
            elif on_gpu and os.environ.get("BH_PT_HOST_EXCHANGE", "0") != "1":
                from .parallel import DeviceExchange, gather_chain_axis
                ladder_all = gather_chain_axis(self.ladder, 0, dist, int(device))
                start = int(sum(self.rank_counts[:self.rank]))         # position of this rank's block in gather order
                mine = slice(start, start + Cn)
                self._dev_exchange = DeviceExchange(ladder_all, self.seed, mine, dev, self.rank_counts)
        self.snap = {"p1": [], "p2": []}

    def window(self):
        """Iterations the next launch may cover: the speculation depth, cut where something outside a chain's own
        state changes -- the proposal-width adaptation (an iteration with iiter % 1000 == 0 is the last of its
        window), a temperature exchange, a snapshot of run(), the end of the run."""
        i = self.iiter
        w = min(self.depth, self.iter_phase2 - i, (-i) % 1000 + 1)
        if self.swap_every > 0 and self.t["beta"] is not None:
            w = min(w, self.swap_every - i % self.swap_every)
        if self.snap_in_run and self._rec is None:     # (the device record: the accept kernel takes the snapshots inside the window)
            w = min(w, self.thinning - i % self.thinning)
        return max(1, w)

    # ---- one lock-step window of all chains: three enqueues, no synchronisation ---------------------
    HINT_EVERY = 64

    def iterate(self):
        """Advance every chain by `window()` iterations (1 with spec_depth = 1); returns that number.
        record="device": the snapshots due inside the window are written by the accept kernel, in run() and in a bare loop of
        iterate() alike (while iiter < iter_main: the store has the rows of a run)."""
        e, t, Cn = self.engine, self.t, self.C
        # transdimensional chains: the dispersion kernel's lane groups and LDS rows are sized for the models the chains
        # hold NOW (typically 5-7 layers in arrays of 21), refreshed every HINT_EVERY launches (one small read-back; run()
        # also does it at every snapshot).  The engine uses it for batches of more than a wavefront's worth of models per
        # SIMD pair (many chains); a window of ~1000 models gets one wavefront per model whatever its depth.
        if self.launches % self.HINT_EVERY == 0:
            # (read on the ENGINE's stream: the accept kernels that write t["n"] run there, not on torch's current stream)
            with self.torch.cuda.stream(self._ext_stream):
                self._hint = int(self.torch.ceil(t["n"].double().mean()).item())
        w = self.window()
        B = Cn * ((1 << w) - 1)
        absent = None if self.absent is None else self.absent.data_ptr()
        rec = self._rec if self.iiter < self.iter_phase2 else None
        if rec is not None:
            rec.row0 = snapshot_count(-self.iter_phase1, self.iiter, self.thinning)
        table = None if self.prior_records is None else (self.prior_records.data_ptr(), self.nsites, self.prior_of.data_ptr())
        propose, propose_extra, accept, accept_extra = window_entries(e, table, rec)
        propose(self.cfg, self.state, Cn, self.iiter, w, self.ld, *propose_extra, absent=absent)
        with e.settings(self.search, self.arith, self.TRIALS, self._hint):   # (for this call only: the engine is shared with other callers)
            if self.sites is not None:
                if e._owner is not self.sites:          # (another caller registered its targets since)
                    self.sites._register()
                e.evaluate_sites_dev(B, self.ML, t["lay_n"].data_ptr(), t["lay_h"].data_ptr(), t["lay_vp"].data_ptr(),
                                     t["lay_vs"].data_ptr(), t["lay_rho"].data_ptr(), self.ld, 1, self.site_map.data_ptr(),
                                     t["pnoise"].data_ptr(), self.logL.data_ptr(), self.mis.data_ptr(), self.err.data_ptr())
            else:
                e.evaluate_batch_dev(B, self.ML, t["lay_n"].data_ptr(), t["lay_h"].data_ptr(), t["lay_vp"].data_ptr(),
                                     t["lay_vs"].data_ptr(), t["lay_rho"].data_ptr(), self.ld, 1, t["pnoise"].data_ptr(),
                                     self.logL.data_ptr(), self.mis.data_ptr(), self.err.data_ptr())
        accept(self.cfg, self.state, Cn, self.iiter, w, self.ld, self.logL.data_ptr(), self.mis.data_ptr(), *accept_extra)
        self.iiter += w
        self.launches += 1
        if self.swap_every > 0 and t["beta"] is not None and self.iiter % self.swap_every == 0:
            self.exchange()
        return w

    def exchange(self):
        """One replica-exchange sweep (the only step of a sharded job with a collective).  On the GPU (one rank, or
        RCCL) it is enqueued on the engine's stream like an iteration (`parallel.DeviceExchange`); with a CPU
        process group (gloo) the gathered values go through the host (`parallel.tempering_exchange`).  With ladder_adapt it
        is one kernel (`parallel.KernelExchange`), which also counts per pair of rungs and, in the burn-in, adapts the ladders."""
        if self.ladder_adapt is not None:
            # a sweep after a window that ends at iiter <= 0 is the burn-in's; the last of every `every` of them adapts
            phase = 0 if self.iiter <= 0 else 1
            every = self.ladder_adapt["every"]
            adapt = phase == 0 and every > 0 and (self.sweep + 1) % every == 0
            with self.torch.cuda.stream(self._ext_stream):
                self._dev_exchange.sweep(self.t["like"], self.t["beta"], self.sweep, phase=phase, adapt=adapt)
            self.sweep += 1
            return
        if self._dev_exchange is not None:
            with self.torch.cuda.stream(self._ext_stream):
                self._dev_exchange.sweep(self.t["like"], self.t["beta"], self.sweep, self.dist)
            self.sweep += 1
            return
        from .parallel import tempering_exchange
        self.engine.synchronize()
        newb, nacc = tempering_exchange(self.t["like"], self.t["beta"], self.ladder, self.sweep, self.seed, self.dist)
        self.t["beta"].copy_(newb)
        self.torch.cuda.synchronize(self.dev)
        self.sweep += 1
        self._nswaps_host += nacc

    @property
    def nswaps(self):
        """accepted swaps so far (all ranks)"""
        return self._nswaps_host + (int(self._dev_exchange.nacc.item()) if self._dev_exchange is not None else 0)

    def ladder_swaps(self):
        """What the exchange sweeps of a run with ladder_adapt proposed and accepted, per neighbouring pair of rungs, and where
        the adaptation left the temperatures.  One dict (SiteTargets: a list of one dict per site, with the site's ladders) of
        `ids` -- the ladder ids --, `members` -- global chain numbers per ladder --, and per ladder of R chains: `betas0` and
        `betas` [R], descending -- the rung values the run started with and holds now --, `proposed` and `accepted` int64
        [2][R-1] -- burn-in, then main phase; pair r is rungs (r, r+1), rung 0 the coldest --, `rate` = accepted / proposed (NaN
        where nothing was proposed); `adaptations` and `skipped` int64 per ladder: the adaptation sweeps that moved the ladder and
        those that left it (a pair without a proposal in the window, or new values out of order).  Waits for the enqueued work.
        EngineError: a run without ladder_adapt."""
        if self.ladder_adapt is None:
            raise EngineError("ladder_swaps() needs DeviceChains(ladder_adapt=...): the default exchange counts accepted swaps only "
                              "(nswaps)")
        ex = self._dev_exchange
        got = ex.plan.read()
        start = ex.plan.start
        out = []
        for ks, members in self._site_ladders(ex.plan.members)[1]:
            d = dict(ids=ex.lids[ks].astype(np.int64), members=members, betas0=[], betas=[], proposed=[], accepted=[], rate=[],
                     adaptations=got["adaptations"][ks], skipped=got["skipped"][ks])
            for k in ks:
                lo, hi = int(start[k]), int(start[k + 1])
                b0 = np.sort(self._betas0[ex.plan.members[k]])[::-1].copy()
                d["betas0"].append(b0)
                d["betas"].append(got["rung_beta"][lo:hi].copy() if ex.nsweeps else b0.copy())
                prop, acc = got["proposed"][:, lo:hi - 1].copy(), got["accepted"][:, lo:hi - 1].copy()
                d["proposed"].append(prop)
                d["accepted"].append(acc)
                with np.errstate(divide="ignore", invalid="ignore"):
                    d["rate"].append(acc / prop.astype(np.float64))
            out.append(d)
        return out if self.sites is not None else out[0]

    def _snapshot(self):
        self.engine.synchronize()
        t = self.t
        row = dict(n=t["n"].cpu().numpy(), vs=t["vs"].cpu().numpy().astype(np.float32),
                   z=t["z"].cpu().numpy().astype(np.float32), like=t["like"].cpu().numpy().astype(np.float32),
                   misfits=t["misfits"].cpu().numpy().astype(np.float32), noise=t["noise"].cpu().numpy().astype(np.float32),
                   vpvs=t["vpvs"].cpu().numpy().astype(np.float32),
                   beta=None if t["beta"] is None else t["beta"].cpu().numpy())
        self.snap["p1" if self.iiter < 0 else "p2"].append(row)
        # transdimensional chains: size the dispersion kernel's lane groups for the models the chains hold now
        self._hint = int(np.ceil(row["n"].mean()))

    def run(self, progress=None):
        self.snap_in_run = True
        try:
            while self.iiter < self.iter_phase2:
                if self._rec is None and self.iiter % self.thinning == 0:
                    self._snapshot()
                before = self.iiter
                self.iterate()
                if progress is not None and self.iiter // 1000 != before // 1000:
                    progress(self)
        finally:
            self.snap_in_run = False
        self.engine.synchronize()
        return self

    # ---- results -------------------------------------------------------------------------------------
    def state_host(self):
        self.engine.synchronize()
        return {k: (None if v is None else v.cpu().numpy()) for k, v in self.t.items()}

    def samples(self, phase="p2", cold_only=False, gather=False, site=None):
        """Thinned samples: dict of arrays with leading axes [nsnap, C]; `models` in the reference's row layout
        [vs_1..vs_n NaN.., z_1..z_n NaN..] (2*maxlayers wide).
        site (SiteTargets): the columns of that site only (its nchains chains; cold_only: its ladders), else all.  With priors
        per site its `models` have the site's own row width, 2*(its layers maximum + 1), as its one-site run returns them;
        without `site` they have the shared width.
        SiteTargets(missing=True): a site's `noise` and `misfits` are in its OWN layout -- the columns of the targets it has,
        as its one-site run returns them; without `site` they are in the slot layout (0 where a site lacks the slot).
        gather: all chains of a sharded job (global chain order) instead of this rank's, on every rank.
        cold_only (tempered runs): one column per LADDER -- at every snapshot the state of the chain holding
        beta = 1; implies gather (the cold chain of a ladder moves between chains, hence between ranks);
        the ladder ids are returned as out["ladder"]."""
        Cn = self.C
        out = self._host_rows(phase) if self._rec is None else self._store_rows(phase)
        if site is not None:
            if self.sites is None:
                raise EngineError("samples(site=...) needs DeviceChains over SiteTargets")
            if not 0 <= int(site) < self.nsites:
                raise IndexError("site %d of %d" % (site, self.nsites))
            out = self._site_block(out, int(site), phase, cold_only, gather)
            out["models"] = out["models"][..., :2 * self.site_ML[int(site)]]   # (n <= the site's capacity: only NaN padding goes)
            if self.present is not None:
                out["noise"], out["misfits"] = gather_slots(self.present[int(site)], out["noise"], out["misfits"])
            return out
        if not (gather or cold_only):
            return out
        from .parallel import gather_chain_axis, cold_samples
        dv = self.dev.index
        out = {k: gather_chain_axis(v, 1, self.dist, dv) for k, v in out.items()}
        out["chain_id"] = gather_chain_axis(self.chain_offset + np.arange(Cn, dtype=np.int64), 0, self.dist, dv)
        if len(np.unique(out["chain_id"])) != out["chain_id"].size:
            raise EngineError("sharded job with overlapping chain numbers (chain_offset): two ranks would draw the same "
                              "random streams and write the same files")
        if cold_only and "beta" in out:
            ladder = gather_chain_axis(self.ladder, 0, self.dist, dv)
            out.pop("chain_id")
            ids, out = cold_samples(out, ladder)
            out["ladder"] = ids
        return out

    def nsamples(self, phase="p2"):
        """snapshots of `phase` taken so far"""
        if self._rec is None:
            return len(self.snap[phase])
        lo, hi = self._store_range(phase)
        return hi - lo

    def _host_rows(self, phase):
        return _host_rows(self.snap[phase], self.C, self.ML, self.nt)

    def _site_block(self, allcols, s, phase, cold_only, gather):
        """samples() of site s: its block of columns (chains s*nchains ..), with gather / cold_only as for all chains"""
        blk = slice(s * self.C_site, (s + 1) * self.C_site)
        out = {k: v[:, blk] for k, v in allcols.items()}
        if not (gather or cold_only):
            return out
        out["chain_id"] = self.chain_offset + np.arange(self.C, dtype=np.int64)[blk]
        if cold_only and "beta" in out:
            from .parallel import cold_samples
            out.pop("chain_id")
            ids, out = cold_samples(out, self.ladder[blk])
            out["ladder"] = ids
        return out

    def save(self, savepath=None):
        """c%03d_p{1,2}{models,likes,misfits,noise,vpvs}.npy, the reference's per-chain result files
        (src/SingleChain.py:646-690), written by rank 0 for ALL chains of the job with their global numbers
        (end-of-run all-gather of the thinned snapshots).  Tempered runs: one file set per ladder, holding the
        beta = 1 samples only (hot chains are not posterior samples)."""
        from .parallel import write_chain_files
        if self.sites is not None:
            return self._save_sites(savepath)
        savepath = op.join(savepath or self.initparams["savepath"], "data")
        tempered = self.t["beta"] is not None
        for tag in ("p1", "p2"):
            if not self.nsamples(tag):
                continue
            s = self.samples(tag, cold_only=tempered, gather=True)      # collective: every rank takes part
            if self.rank == 0:
                # file numbers = GLOBAL chain indices (= the chain's Philox / initial-state index), also with an
                # explicit chain_offset; tempered runs: ladder ids
                ids = s["ladder"] if tempered else s["chain_id"]
                write_chain_files(savepath, tag, s, ids)
        if self.rank == 0:
            from .results import save_config
            save_config(self.targets, op.join(savepath, "%s_config.pkl" % self.initparams.get("station", "test")),
                        priors=self.priors, initparams=self.initparams)
        if self.dist is not None and self.dist.is_initialized() and self.dist.get_world_size() > 1:
            self.dist.barrier()
        return savepath

    def _save_sites(self, savepath=None):
        """SiteTargets: one reference-format folder per site, <savepath>/<name>/data/ with the chain files of that site's
        chains (global numbers, as a one-site run with chain_offset = s*nchains writes them) and <name>_config.pkl built
        from that site's targets.  Returns the list of data folders."""
        from .parallel import write_chain_files
        from .results import save_config
        root = savepath or self.initparams["savepath"]
        tempered = self.t["beta"] is not None
        out = []
        for s, name in enumerate(self.sites.names):
            datapath = op.join(root, name, "data")
            for tag in ("p1", "p2"):
                if not self.nsamples(tag):
                    continue
                smp = self.samples(tag, cold_only=tempered, gather=True, site=s)
                write_chain_files(datapath, tag, smp, smp["ladder"] if tempered else smp["chain_id"])
            ip = dict(self.site_initparams[s], station=name, savepath=op.join(root, name))
            save_config(self.sites.site(s), op.join(datapath, "%s_config.pkl" % name), priors=self.site_priors[s], initparams=ip)
            out.append(datapath)
        return out
