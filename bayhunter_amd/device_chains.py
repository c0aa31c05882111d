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

import numpy as np

from .chains import ChainBatch, DEFAULT_INITPARAMS, DEFAULT_PRIORS, _is_fixed
from .engine import BH_CHAIN_MAXDEPTH, BH_CHAIN_MAXLAYERS, ChainConfig, ChainPrior, ChainRecord, ChainState, EngineError
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


class DeviceChains(object):
    TRIALS = 32  # trials per round of the trial-per-lane kernel in every evaluation call of the chains (windows and initial state)

    def __init__(self, targets, nchains, initparams=None, modelpriors=None, seed=0, device=None, inject=False,
                 betas=None, ladder=None, swap_every=0, dist=None, chain_offset=None, spec_depth=None, search="fast", arith="fast",
                 prior_table=False, record="host", ladder_adapt=None):
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
        if record not in RECORD_MODES:      # (checked before anything touches the GPU)
            raise ValueError("record must be 'host' or 'device', not %r" % (record,))
        self.record = record
        self.ladder_adapt = ladder_adapt_options(ladder_adapt, betas, ladder, swap_every, dist)
        self.sites = targets if isinstance(targets, SiteTargets) else None
        self.nsites = 1 if self.sites is None else self.sites.nsites
        if self.sites is None:   # (SiteTargets refuses it itself: "a user plugin")
            from .Targets import RayleighEllipticity
            for t in (targets.targets if isinstance(targets, JointTarget) else targets):
                if isinstance(t, RayleighEllipticity) and not t.engine_backed():   # (fused=True: part of the fused call)
                    raise EngineError("DeviceChains does not run RayleighEllipticity: the device chains evaluate engine-backed "
                                      "targets in one fused call, and the ellipticity is not part of it yet (ChainBatch runs it)")
        # (checked before anything touches the GPU)
        self.site_initparams, self.site_priors, differ = site_dicts(initparams, modelpriors, self.nsites, self.sites is not None)
        if prior_table and self.sites is None:
            raise ValueError("prior_table=True needs SiteTargets")
        self.prior_table = bool(differ or prior_table)
        import torch
        self.torch = torch
        if self.sites is not None and dist is not None:
            raise EngineError("DeviceChains with SiteTargets does not shard: give each process its own sites instead of dist")
        self.targets = targets if isinstance(targets, (JointTarget, SiteTargets)) else JointTarget(targets)
        if self.targets._engine is None and device is not None:
            from .engine import default_engine
            self.targets._engine = default_engine(int(device))   # kernels and tensors on the same GPU
        self.engine = self.targets.engine
        if search not in (None, "reference", "fast", "fast_rayleigh"):
            raise ValueError("search must be None, 'reference', 'fast' or 'fast_rayleigh'")
        self.search = search
        if arith not in (None, "exact", "fast"):
            raise ValueError("arith must be None, 'exact' or 'fast'")
        self.arith = arith
        if device is None:
            device = self.engine.device
        if int(device) != int(self.engine.device):
            raise EngineError("DeviceChains(device=%d) but the targets' engine runs on GPU %d" % (device, self.engine.device))
        self.initparams, self.priors = self.site_initparams[0], self.site_priors[0]
        ip, pr = self.initparams, self.priors
        self.C_site = int(nchains)                        # chains per site (sites: S blocks of them, site after site)
        self.C = self.C_site * self.nsites
        self.nt = self.targets.ntargets
        self.site_ML = [int(p["layers"][1]) + 1 for p in self.site_priors]   # a site's own row capacity
        self.ML = max(self.site_ML)                       # rows of the arrays: the largest
        self.iter_phase1, self.iter_phase2 = int(ip["iter_burnin"]), int(ip["iter_main"])
        self.iterations = self.iter_phase1 + self.iter_phase2
        self.iiter = -self.iter_phase1
        self.thinning = max(1, int(np.ceil(float(self.iter_phase2) / float(ip["maxmodels"]))))
        self.swap_every, self.dist, self._nswaps_host, self.sweep, self.seed = int(swap_every), dist, 0, 0, int(seed)
        self.depth = auto_spec_depth(self.C) if spec_depth is None else int(spec_depth)
        if not 1 <= self.depth <= BH_CHAIN_MAXDEPTH:
            raise EngineError("spec_depth must be 1..%d" % BH_CHAIN_MAXDEPTH)
        self.ld = self.C * ((1 << self.depth) - 1)        # columns of the proposal arrays: all nodes of all chains
        self.snap_in_run = False                          # run(): windows also end at snapshot iterations
        self.launches = 0
        self._hint = 0
        self._dev_exchange = None
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
        self.present = None if self.sites is None or not self.sites.missing else self.sites.present
        if self.prior_table:   # per site, in the slot layout; a slot the site lacks: fixed (and masked by `absent`)
            self.noisepriors = None
            self.site_noisepriors = []
            for s, h in enumerate(hosts):
                have = np.arange(self.nt) if self.present is None else np.flatnonzero(self.present[s])
                row = [0.0] * (2 * self.nt)
                for j, i in enumerate(have):
                    row[2 * i], row[2 * i + 1] = h.noisepriors[2 * j], h.noisepriors[2 * j + 1]
                self.site_noisepriors.append(row)
        elif self.present is None:
            self.noisepriors = hosts[0].noisepriors
            if any(h.noisepriors != self.noisepriors for h in hosts):
                raise EngineError("the sites' noise priors differ")
        else:   # slot by slot, among the sites that have the slot (a site's own list holds its present targets' only)
            self.noisepriors = [None] * (2 * self.nt)
            for s, h in enumerate(hosts):
                for j, i in enumerate(np.flatnonzero(self.present[s])):
                    for k in (0, 1):
                        if self.noisepriors[2 * i + k] is None:
                            self.noisepriors[2 * i + k] = h.noisepriors[2 * j + k]
                        elif self.noisepriors[2 * i + k] != h.noisepriors[2 * j + k]:
                            raise EngineError("the sites' noise priors differ")
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
            set_station_fields(cfg, ip, pr, self.noisepriors)
        cfg.seed = int(seed) & (2 ** 64 - 1)
        cfg.chain_offset = off
        self.cfg = cfg

        dev = torch.device("cuda", int(device))
        self.dev = dev
        Cn, ML, nt = self.C, self.ML, self.nt
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        t = {}
        vs0 = np.zeros((ML, Cn)); z0 = np.zeros((ML, Cn)); n0 = np.zeros(Cn, dtype=np.int32)
        noise0 = np.zeros((2 * nt, Cn)); mis0 = np.zeros((nt + 1, Cn))
        like0 = np.zeros(Cn); vpvs0 = np.zeros(Cn); pd0 = np.zeros((5, Cn))
        for c, ch in enumerate(host_chains):
            m = np.asarray(ch.currentmodel, dtype=float)
            n = m.size // 2
            n0[c] = n
            vs0[:n, c], z0[:n, c] = m[:n], m[n:]
            if self.present is None:
                noise0[:, c], mis0[:, c] = ch.currentnoise, ch.currentmisfits
            else:   # the site's own layout into the slot layout
                noise0[:, c], mis0[:, c] = scatter_slots(self.present[c // self.C_site], ch.currentnoise, ch.currentmisfits)
            like0[c], vpvs0[c] = ch.currentlikelihood, ch.currentvpvs
            pd0[:, c] = ch.propdist
        t["n"] = torch.from_numpy(n0).to(dev)
        t["vs"], t["z"] = torch.from_numpy(vs0).to(dev), torch.from_numpy(z0).to(dev)
        t["vpvs"], t["noise"] = torch.from_numpy(vpvs0).to(dev), torch.from_numpy(noise0).to(dev)
        t["like"], t["misfits"] = torch.from_numpy(like0).to(dev), torch.from_numpy(mis0).to(dev)
        t["propdist"] = torch.from_numpy(pd0).to(dev)
        t["proposed"], t["accepted"] = torch.zeros((5, Cn), **f64), torch.zeros((5, Cn), **f64)
        t["naccepted"] = torch.zeros(Cn, dtype=torch.int64, device=dev)
        t["beta"] = None if betas is None else torch.as_tensor(np.asarray(betas, dtype=np.float64)).to(dev)
        self.ladder = None if betas is None else np.asarray(ladder if ladder is not None else np.zeros(Cn), dtype=np.int64)
        self.site_map = None
        if self.sites is not None:
            if self.ladder is not None:
                of = np.arange(Cn) // self.C_site
                for lid in np.unique(self.ladder):
                    if np.unique(of[self.ladder == lid]).size > 1:
                        raise EngineError("tempering ladder %d spans sites: every ladder must lie within one site" % lid)
            self.site_map = torch.from_numpy(window_site_map(self.C_site, self.nsites, self.ld)).to(dev)
        # (missing=True) per chain, bit i set: the chain's site lacks slot i -- its noise parameters are not free there
        self.absent = None
        if self.present is not None:
            bits = ((~self.present).astype(np.int64) << np.arange(nt)).sum(axis=1).astype(np.uint8)
            self.absent = torch.from_numpy(np.repeat(bits, self.C_site)).to(dev)
        # (priors per site) the table of records and, per chain, its site's record
        self.prior_records = self.prior_of = None
        if records is not None:
            self.prior_records = torch.from_numpy(np.frombuffer(records, dtype=np.uint8).copy()).to(dev)
            self.prior_of = torch.from_numpy(np.repeat(np.arange(self.nsites, dtype=np.int32), self.C_site)).to(dev)
        ld = self.ld                                      # node j of chain c in column j*C + c
        for k in ("pn", "move", "valid", "lay_n"):
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

    def _allocate_store(self, tempered):
        """the device store of record="device": every row of both phases (include/bh_engine_chain_record.h)"""
        torch, Cn, ML, nt = self.torch, self.C, self.ML, self.nt
        rows = sum(record_rows(self.iter_phase1, self.iter_phase2, self.thinning))
        shapes = dict(models=(rows, Cn, 2 * ML), likes=(rows, Cn), vpvs=(rows, Cn), misfits=(rows, Cn, nt + 1), noise=(rows, Cn, 2 * nt))
        need = 4 * sum(int(np.prod(sh)) for sh in shapes.values()) + (8 * rows * Cn if tempered else 0)
        free = torch.cuda.mem_get_info(self.dev)[0]
        if need > free:
            raise EngineError("record='device': the store of %d rows x %d chains takes %.2f GiB, %.2f GiB are free on GPU %d "
                              "(maxmodels = %s gives thinning %d: lower maxmodels, or record='host')"
                              % (rows, Cn, need / 2.0 ** 30, free / 2.0 ** 30, self.dev.index, self.initparams["maxmodels"], self.thinning))
        self.store = {k: torch.empty(sh, dtype=torch.float32, device=self.dev) for k, sh in shapes.items()}
        self.store["beta"] = torch.empty((rows, Cn), dtype=torch.float64, device=self.dev) if tempered else None
        rec = ChainRecord()
        for k, v in self.store.items():
            setattr(rec, k, None if v is None else v.data_ptr())
        rec.rows, rec.thinning, rec.row0 = rows, self.thinning, 0
        self._rec = rec

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
        e.set_typical_layers(self._hint)       # (for this call only: the engine is shared with other callers)
        prev = e.swd_search() if self.search is not None else None
        if prev is not None and prev != self.search:
            e.set_swd_search(self.search)
        prev_arith, prev_trials = (e.swd_arith() if self.arith is not None else None), e.swd_trials()
        if prev_arith is not None and prev_arith != self.arith:
            e.set_swd_arith(self.arith)
        e.set_swd_trials(self.TRIALS)
        try:
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
        finally:
            e.set_typical_layers(0)
            if prev is not None and prev != self.search:
                e.set_swd_search(prev)
            if prev_arith is not None and prev_arith != self.arith:
                e.set_swd_arith(prev_arith)
            e.set_swd_trials(prev_trials)
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
        for s in range(self.nsites):
            ks = [k for k in range(ex.plan.K) if ex.plan.members[k][0] // self.C_site == s]
            d = dict(ids=ex.lids[ks].astype(np.int64), members=[self.chain_offset + ex.plan.members[k].astype(np.int64) for k in ks],
                     betas0=[], betas=[], proposed=[], accepted=[], rate=[],
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

    def _store_range(self, phase):
        """rows [lo, hi) of the device store that hold the snapshots of `phase` taken so far (up to the current iiter)"""
        if phase not in ("p1", "p2"):
            raise KeyError(phase)
        r1 = record_rows(self.iter_phase1, self.iter_phase2, self.thinning)[0]
        done = snapshot_count(-self.iter_phase1, min(self.iiter, self.iter_phase2), self.thinning)
        return (0, min(done, r1)) if phase == "p1" else (r1, max(done, r1))

    def _store_rows(self, phase):
        """the rows of samples() from the device store: one copy per array"""
        lo, hi = self._store_range(phase)
        self.engine.synchronize()
        out = {k: self.store[k][lo:hi].cpu().numpy() for k in ("models", "likes", "vpvs", "misfits", "noise")}
        if hi > lo and self.store["beta"] is not None:
            out["beta"] = self.store["beta"][lo:hi].cpu().numpy()
        return out

    def samples_dev(self, phase="p2", cold_only=False, exclude_chains=()):
        """record="device": the snapshots of `phase` taken so far where the accept kernel wrote them -- a dict of torch views of
        the store, models [rows, C, 2*maxlayers], likes / vpvs [rows, C], misfits [rows, C, nt+1], noise [rows, C, 2nt] (float32,
        all chains, shared row width and slot layout), tempered runs also beta [rows, C] (float64); and, for the posterior kernels,
        models2d = the [rows*C, 2*maxlayers] view of the models and site = int32 [rows*C], every row's site index:
        posterior_models(d["models2d"], site=d["site"], nsites=...) summarises them without a host copy.  Waits for the engine's
        stream (the posterior kernels run on torch's).
        cold_only (tempered runs): the rows that are no posterior samples -- at every snapshot every chain but the one holding
        beta = 1 in its ladder (the first of the largest beta, as samples(cold_only=True) picks it) -- get site = -1, which the
        posterior kernels leave out and count as dropped.  exclude_chains: chain numbers (outliers) whose rows get site = -1 too.
        Both are formed on the device; the views of the store still hold every row."""
        if self._rec is None:
            raise EngineError("samples_dev() needs DeviceChains(record='device')")
        torch = self.torch
        lo, hi = self._store_range(phase)
        self.engine.synchronize()
        out = {k: v[lo:hi] for k, v in self.store.items() if v is not None}
        out["models2d"] = out["models"].reshape((hi - lo) * self.C, 2 * self.ML)
        of = torch.arange(self.C, dtype=torch.int32, device=self.dev) // self.C_site
        site = of.repeat(hi - lo)
        exclude = np.atleast_1d(np.asarray(exclude_chains, dtype=np.int64)) - self.chain_offset
        if exclude.size and (exclude.min() < 0 or exclude.max() >= self.C):
            raise IndexError("exclude_chains: chain numbers %d..%d" % (self.chain_offset, self.chain_offset + self.C - 1))
        if (cold_only and "beta" in out) or exclude.size:
            keep = torch.ones((hi - lo, self.C), dtype=torch.bool, device=self.dev)
            if cold_only and "beta" in out:
                keep &= self._cold_mask(out["beta"])
            if exclude.size:
                keep[:, torch.from_numpy(exclude).to(self.dev)] = False
            site = torch.where(keep.reshape(-1), site, torch.full_like(site, -1))
        out["site"] = site
        return out

    def _cold_mask(self, beta):
        """bool [rows, C]: at every snapshot, the chain of every ladder that cold_samples() picks (the first of the largest beta)"""
        torch = self.torch
        if self.dist is not None and self.dist.is_initialized() and self.dist.get_world_size() > 1:
            raise EngineError("samples_dev(cold_only=True) does not follow ladders across ranks: use samples(cold_only=True)")
        rows, Cn = beta.shape
        lad = torch.from_numpy(np.unique(self.ladder, return_inverse=True)[1].astype(np.int64)).to(self.dev)
        nl = int(lad.max().item()) + 1 if Cn else 0
        idx = lad.expand(rows, Cn)
        top = torch.full((rows, nl), -np.inf, dtype=beta.dtype, device=self.dev).scatter_reduce(1, idx, beta, "amax")
        chain = torch.arange(Cn, dtype=torch.int64, device=self.dev).expand(rows, Cn)
        cand = torch.where(beta == top.gather(1, idx), chain, torch.full_like(chain, Cn))
        first = torch.full((rows, nl), Cn, dtype=torch.int64, device=self.dev).scatter_reduce(1, idx, cand, "amin")
        return chain == first.gather(1, idx)

    def _posterior_rows(self, phase, cold_only, exclude_chains):
        if self._rec is None:
            raise EngineError("samples_dev() needs DeviceChains(record='device')")
        if cold_only is None:
            cold_only = self.ladder is not None
        return self.samples_dev(phase, cold_only=cold_only, exclude_chains=exclude_chains)

    def _class_rows(self, classes, phase, cold_only, exclude_chains):
        """classes= of the posterior_* methods: the dict must stem from the same selection of the store's rows"""
        if classes is None:
            return None
        if cold_only is None:
            cold_only = self.ladder is not None
        sel = (phase, bool(cold_only), tuple(int(c) for c in np.atleast_1d(np.asarray(exclude_chains, dtype=np.int64))))
        if not isinstance(classes, dict) or "selection" not in classes:
            raise ValueError("classes must be the dict DeviceChains.posterior_classes returned")
        if tuple(classes["selection"]) != sel:
            raise ValueError("classes was formed with (phase, cold_only, exclude_chains) = %r, this call asks for %r: classify "
                             "the same rows" % (tuple(classes["selection"]), sel))
        return classes

    def posterior_classes(self, classes, features=None, moho=None, mohovs=4.2, scalars=(), phase="p2", cold_only=None, exclude_chains=()):
        """record="device": bayhunter_amd.posterior_classes of every site's recorded rows where they lie in the device store: every
        row's class by a rule over its scalar columns -- classes: name -> list of (label, lo, hi), (label, "has"), (label, "lacks"),
        the first class that holds taking the row.  Labels: those of features (name -> (kind, z0, z1[, c])); "moho", "vslast",
        "vscrust", "vsjump" with moho = (lo, hi) (True: every site's own priors['z']) and mohovs; and of scalars, names of the store's
        columns as posterior_covariance() takes them -- "likes", "vpvs", "misfits[i]", "noise[i]" -- and "nlayers".  cold_only
        (default: True on tempered runs) and exclude_chains as in samples_dev().  The dict (cls, counts, probability, ...: see
        bayhunter_amd.posterior_classes; cls and site are device tensors over the rows of samples_dev()) remembers the selection
        (phase, cold_only, exclude_chains); classes= of the posterior_* methods takes it with the same selection only."""
        from .posterior import posterior_classes
        d = self._posterior_rows(phase, cold_only, exclude_chains)
        n = d["models2d"].shape[0]
        shapes = dict(likes=(n,), vpvs=(n,), misfits=(n, self.nt + 1), noise=(n, 2 * self.nt))
        if isinstance(scalars, str):
            scalars = (scalars,)
        unknown = [k for k in scalars if k not in shapes and k != "nlayers"]
        if unknown:
            raise ValueError("scalars: %r is no column of the store (%s, nlayers)" % (unknown[0], ", ".join(shapes)))
        cols = {k: d[k].reshape(shapes[k]) for k in scalars if k != "nlayers"}
        if moho is True:
            moho = [tuple(float(v) for v in p["z"]) for p in self.site_priors]
        with self.torch.cuda.device(self.dev):
            r = posterior_classes(d["models2d"], classes, site=d["site"], features=features, moho=moho, mohovs=mohovs,
                                  columns=cols or None, nlayers="nlayers" in scalars, engine=self.engine, nsites=self.nsites)
        if cold_only is None:
            cold_only = self.ladder is not None
        r["selection"] = (phase, bool(cold_only), tuple(int(c) for c in np.atleast_1d(np.asarray(exclude_chains, dtype=np.int64))))
        return r

    def posterior_models(self, dep_int=None, quantiles=None, phase="p2", cold_only=None, exclude_chains=(), classes=None):
        """record="device": bayhunter_amd.posterior_models of every site's recorded rows, straight from the device store (one dict
        per site; one dict without SiteTargets): mean, median, minmax, stdminmax, mode and -- the joint misfit misfits[..., -1]
        being in the store -- minmisfit of vs against depth; quantiles (numbers in [0, 1]) adds the credible band `quantiles`.
        cold_only (default: True on tempered runs) and exclude_chains as in samples_dev().  classes: the dict
        posterior_classes() returned for the same phase, cold_only and exclude_chains: per site a dict class name -> that dict."""
        classes = self._class_rows(classes, phase, cold_only, exclude_chains)
        from .posterior import posterior_models
        d = self._posterior_rows(phase, cold_only, exclude_chains)
        n = d["models2d"].shape[0]
        with self.torch.cuda.device(self.dev):
            r = posterior_models(d["models2d"], site=d["site"], dep_int=dep_int, misfits=d["misfits"][..., -1].reshape(n),
                                 engine=self.engine, nsites=self.nsites, quantiles=quantiles, classes=classes)
        return r if self.sites is not None else r[0]

    def posterior_hist2d(self, dep_int=None, vs_edges=None, dep_edges=None, phase="p2", cold_only=None, exclude_chains=(), classes=None):
        """record="device": bayhunter_amd.posterior_hist2d of every site's recorded rows, straight from the device store (one dict
        per site; one dict without SiteTargets): the 2-D posterior plot's vs-depth histogram and the histogram of interface
        depths.  cold_only (default: True on tempered runs) and exclude_chains as in samples_dev().  classes: the dict
        posterior_classes() returned for the same phase, cold_only and exclude_chains: per site a dict class name -> that dict."""
        classes = self._class_rows(classes, phase, cold_only, exclude_chains)
        from .posterior import posterior_hist2d
        d = self._posterior_rows(phase, cold_only, exclude_chains)
        with self.torch.cuda.device(self.dev):
            r = posterior_hist2d(d["models2d"], site=d["site"], dep_int=dep_int, vs_edges=vs_edges, dep_edges=dep_edges,
                                 engine=self.engine, nsites=self.nsites, classes=classes)
        return r if self.sites is not None else r[0]

    def posterior_moho(self, moho=None, mohovs=4.2, bins=50, phase="p2", cold_only=None, exclude_chains=(), quantiles=None, classes=None):
        """record="device": bayhunter_amd.posterior_moho of every site's recorded rows, straight from the device store (one dict
        per site; one dict without SiteTargets).  moho None: every site's own priors['z'], the reference's default.  cold_only
        (default: True on tempered runs) and exclude_chains as in samples_dev().  quantiles: as posterior_moho's.  classes: the dict
        posterior_classes() returned for the same phase, cold_only and exclude_chains: per site a dict class name -> that dict."""
        classes = self._class_rows(classes, phase, cold_only, exclude_chains)
        from .posterior import posterior_moho
        d = self._posterior_rows(phase, cold_only, exclude_chains)
        if moho is None:
            moho = [tuple(float(v) for v in p["z"]) for p in self.site_priors]
        with self.torch.cuda.device(self.dev):
            r = posterior_moho(d["models2d"], site=d["site"], moho=moho, mohovs=mohovs, bins=bins, engine=self.engine,
                               nsites=self.nsites, quantiles=quantiles, classes=classes)
        return r if self.sites is not None else r[0]

    def posterior_features(self, features, bins=50, phase="p2", cold_only=None, exclude_chains=(), quantiles=None, classes=None):
        """record="device": bayhunter_amd.posterior_features of every site's recorded rows, straight from the device store (one dict
        per site; one dict without SiteTargets): the posteriors of structural features of the layered models -- features: name ->
        (kind, z0, z1[, c]), every number one value or one per site.  cold_only (default: True on tempered runs) and
        exclude_chains as in samples_dev().  quantiles: as posterior_features'.  classes: the dict
        posterior_classes() returned for the same phase, cold_only and exclude_chains: per site a dict class name -> that dict."""
        classes = self._class_rows(classes, phase, cold_only, exclude_chains)
        from .posterior import posterior_features
        d = self._posterior_rows(phase, cold_only, exclude_chains)
        with self.torch.cuda.device(self.dev):
            r = posterior_features(d["models2d"], features, site=d["site"], bins=bins, quantiles=quantiles, engine=self.engine,
                                   nsites=self.nsites, classes=classes)
        return r if self.sites is not None else r[0]

    def posterior_scalars(self, bins=20, nlayers=True, phase="p2", cold_only=None, exclude_chains=(), quantiles=None, classes=None):
        """record="device": bayhunter_amd.posterior_scalars of every site's recorded rows with the store's likes, vpvs, misfits
        [nt+1] and noise [2nt] as columns (slot layout), straight from the device store (one dict per site; one dict without
        SiteTargets).  cold_only (default: True on tempered runs) and exclude_chains as in samples_dev().  quantiles: as
        posterior_scalars'.  classes: the dict
        posterior_classes() returned for the same phase, cold_only and exclude_chains: per site a dict class name -> that dict."""
        classes = self._class_rows(classes, phase, cold_only, exclude_chains)
        from .posterior import posterior_scalars
        d = self._posterior_rows(phase, cold_only, exclude_chains)
        n = d["models2d"].shape[0]
        cols = dict(likes=d["likes"].reshape(n), vpvs=d["vpvs"].reshape(n), misfits=d["misfits"].reshape(n, self.nt + 1),
                    noise=d["noise"].reshape(n, 2 * self.nt))
        with self.torch.cuda.device(self.dev):
            r = posterior_scalars(d["models2d"], cols, site=d["site"], bins=bins, nlayers=nlayers, engine=self.engine,
                                  nsites=self.nsites, quantiles=quantiles, classes=classes)
        return r if self.sites is not None else r[0]

    def posterior_covariance(self, dep_int=None, scalars=(), moho=None, mohovs=4.2, phase="p2", cold_only=None, exclude_chains=(),
                             features=None, classes=None):
        """record="device": bayhunter_amd.posterior_covariance of every site's recorded rows, straight from the device store (one
        dict per site; one dict without SiteTargets): mean, covariance and correlation of vs at the depths of dep_int.  scalars:
        names of the store's columns to put beside the depths -- likes, vpvs, misfits [nt+1] and noise [2nt], as
        posterior_scalars() takes them; or moho = (lo, hi) (True: every site's own priors['z']) with mohovs for the Moho depth and
        the mean crustal vs; or features: name -> (kind, z0, z1[, c]) as posterior_features() takes them -- one of the three.  cold_only
        (default: True on tempered runs) and exclude_chains as in samples_dev().  classes: the dict
        posterior_classes() returned for the same phase, cold_only and exclude_chains: per site a dict class name -> that dict."""
        classes = self._class_rows(classes, phase, cold_only, exclude_chains)
        from .posterior import posterior_covariance
        d = self._posterior_rows(phase, cold_only, exclude_chains)
        n = d["models2d"].shape[0]
        shapes = dict(likes=(n,), vpvs=(n,), misfits=(n, self.nt + 1), noise=(n, 2 * self.nt))
        if isinstance(scalars, str):
            scalars = (scalars,)
        unknown = [k for k in scalars if k not in shapes]
        if unknown:
            raise ValueError("scalars: %r is no column of the store (%s)" % (unknown[0], ", ".join(shapes)))
        cols = {k: d[k].reshape(shapes[k]) for k in scalars} if len(scalars) else None
        if moho is True:
            moho = [tuple(float(v) for v in p["z"]) for p in self.site_priors]
        with self.torch.cuda.device(self.dev):
            r = posterior_covariance(d["models2d"], site=d["site"], dep_int=dep_int, columns=cols, moho=moho, mohovs=mohovs,
                                     engine=self.engine, nsites=self.nsites, features=features, classes=classes)
        return r if self.sites is not None else r[0]

    def posterior_datafits(self, quantiles=(0.025, 0.16, 0.5, 0.84, 0.975), phase="p2", cold_only=None, exclude_chains=()):
        """record="device": bayhunter_amd.posterior_datafits of every site's recorded rows, straight from the device store (one
        dict per site; one dict without SiteTargets): the best fit of every chain -- the chain id is the row's column in the
        store, misfits[..., -1] the joint misfit -- and the predictive band of every datum; every site's mantle rule is that of
        its priors.  cold_only (default: True on tempered runs) and exclude_chains as in samples_dev()."""
        from .datafits import posterior_datafits
        d = self._posterior_rows(phase, cold_only, exclude_chains)
        n = d["models2d"].shape[0]
        chain = self.torch.arange(self.C, dtype=self.torch.int32, device=self.dev).repeat(n // self.C if self.C else 0)
        targets = self.sites if self.sites is not None else self.targets
        mantle = [p.get("mantle") for p in self.site_priors]
        with self.torch.cuda.device(self.dev):
            return posterior_datafits(targets, d["models2d"], d["vpvs"].reshape(n), site=d["site"], chain=chain,
                                      misfits=d["misfits"][..., -1].reshape(n), quantiles=quantiles, mantle=mantle,
                                      engine=self.engine)

    def posterior_residuals(self, maxlag=10, quantiles=(0.025, 0.16, 0.5, 0.84, 0.975), phase="p2", cold_only=None, exclude_chains=()):
        """record="device": bayhunter_amd.posterior_residuals of every site's recorded rows, straight from the device store (one
        dict per site; one dict without SiteTargets): whether the residuals of the recorded models look like the noise each row
        assumed -- the store's noise table [2nt] (slot layout) is read where it lies; every site's mantle rule is that of its
        priors.  cold_only (default: True on tempered runs) and exclude_chains as in samples_dev()."""
        from .datafits import posterior_residuals
        d = self._posterior_rows(phase, cold_only, exclude_chains)
        n = d["models2d"].shape[0]
        targets = self.sites if self.sites is not None else self.targets
        mantle = [p.get("mantle") for p in self.site_priors]
        with self.torch.cuda.device(self.dev):
            return posterior_residuals(targets, d["models2d"], d["vpvs"].reshape(n), d["noise"].reshape(n, 2 * self.nt), site=d["site"],
                                       maxlag=maxlag, quantiles=quantiles, mantle=mantle, engine=self.engine)

    def diagnostics(self, phase="p2", dep=None, maxlag=None, dev=0.05, exclude_chains=None, rank=False, features=None, moho=None,
                    mohovs=4.2):
        """record="device": bayhunter_amd.diagnostics of every site's chains, straight from the time-ordered views of the device
        store (one dict per site; one dict without SiteTargets): `outliers` -- the global numbers of the chains the reference's rule
        (results.get_outliers, deviation `dev`) rejects, ready to pass as exclude_chains= to the posterior_* methods --, their
        `scores`, and for likes, vpvs, misfits [nt+1], noise [2nt] (slot layout), nlayers and vs (at the depths `dep`, default
        np.linspace(0, 100, 41)) the dict of diagnostics.convergence: split R-hat, ESS, tau, the flags and the per-chain numbers.
        exclude_chains None: R-hat and ESS over the chains that are no outliers; a sequence of chain numbers overrides that.
        maxlag: the largest lag of the autocorrelation sums, default min(T // 2, 1000).
        rank=True: every group's dict gains "rank" -- the rank-normalised and the folded split R-hat, the bulk and the tail ESS of
        diagnostics.rank_convergence, the site's kept chains pooled on the GPU; with the default nothing of it runs.
        features (the dict of posterior_features, every number a scalar or one per site) and / or moho = (lo, hi) or one pair per
        site, with mohovs (the feature "moho", posterior_moho's depth column): every site's dict gains "features", the dict of
        diagnostics.feature_convergence -- R-hat, ESS and the Monte-Carlo standard error of every feature column (mcse_mean), the
        probability that a row has it and its own error (presence, mcse_probability) -- from series the GPU forms out of the model
        rows where they lie; with the defaults nothing of it runs.
        EngineError: record="host" (no time-ordered store on the GPU), a tempered run (a ladder's cold state moves between chains:
        no chain's series is a posterior series) and a sharded job of more than one rank (a site's chains lie on several GPUs)."""
        if self._rec is None:
            raise EngineError("diagnostics() needs DeviceChains(record='device'): record='host' keeps no time-ordered store of the "
                              "chains on the GPU (results.diagnostics_from_storage reads saved folders)")
        if self.t["beta"] is not None:
            raise EngineError("diagnostics() of a tempered run: a ladder's cold state moves between chains, so no chain's recorded "
                              "series is a series of posterior samples")
        if self.dist is not None and self.dist.is_initialized() and self.dist.get_world_size() > 1:
            raise EngineError("diagnostics() of a sharded job (world size %d): the chains of a site lie on several ranks"
                              % self.dist.get_world_size())
        from .diagnostics import diagnose
        d = self.samples_dev(phase)
        if not d["likes"].shape[0]:
            raise EngineError("diagnostics(): no snapshot of phase %r yet" % (phase,))
        ids = self.chain_offset + np.arange(self.C, dtype=np.int64)
        with self.torch.cuda.device(self.dev):
            r = diagnose(d, np.arange(self.C) // self.C_site, ids, dev=dev, dep=dep, maxlag=maxlag, exclude_chains=exclude_chains,
                         engine=self.engine, rank=rank, features=features, moho=moho, mohovs=mohovs)
        return r if self.sites is not None else r[0]

    def ladder_diagnostics(self, phase="p2", dep=None, maxlag=None, dev=0.05, exclude_ladders=None, rank=False, features=None,
                           moho=None, mohovs=4.2):
        """record="device", tempered runs: bayhunter_amd.diagnostics of every site's LADDERS, straight from the device store.  The
        posterior series of a ladder is its cold series -- at every recorded row the state of the chain that holds the ladder's
        largest beta (the first of them: what samples(cold_only=True) and save() pick); diagnostics.ladder_index finds that chain
        on the GPU from the recorded betas and the sums read it where the rows lie, with the bits of diagnostics.diagnose on
        samples(phase, cold_only=True).  One dict per site (one dict without SiteTargets), shaped as diagnostics() returns it with
        ladders where chains were: `outliers` -- the ids of the ladders the reference's rule rejects on the cold series' median
        likelihood --, `outlier_chains` -- the global chain numbers of all members of those ladders, ready to pass as
        exclude_chains= to the posterior_* methods --, `scores`, `chain_ids` (the site's ladder ids), and the convergence dicts of
        likes, vpvs, misfits, noise, nlayers and vs, whose `chains` are ladder ids; and `ladders` = dict of ids, members (global
        chain numbers per ladder), moves (changes of the cold holder per ladder), and per chain of the site, in chain order:
        chains (their global numbers), round_trips (cold -> hot -> cold excursions seen at the recorded rows), occupancy [.][R]
        (rows spent on every rung) and cold_share = occupancy[:, 0] / T.
        exclude_ladders None: R-hat and ESS over the ladders that are no outliers; a sequence of ladder ids overrides that.
        features, moho, mohovs: as diagnostics() -- "features" of every site from the feature series of the ladders' cold series,
        read in place; its `chains` are ladder ids.
        EngineError: record="host", an untempered run (use diagnostics()), a sharded job of more than one rank (ladders are not
        followed across ranks).  ValueError: rank=True -- the ranks of cold series are not formed."""
        if rank:
            raise ValueError("ladder_diagnostics(rank=True): the ranks of the cold series of tempered runs are not formed")
        if self._rec is None:
            raise EngineError("ladder_diagnostics() needs DeviceChains(record='device'): record='host' keeps no time-ordered store of "
                              "the chains on the GPU (results.diagnostics_from_storage reads saved folders)")
        if self.t["beta"] is None or self.ladder is None:
            raise EngineError("ladder_diagnostics() of an untempered run: there are no ladders -- every chain's own series is a "
                              "posterior series, use diagnostics()")
        if self.dist is not None and self.dist.is_initialized() and self.dist.get_world_size() > 1:
            raise EngineError("ladder_diagnostics() does not follow ladders across ranks (world size %d): use "
                              "samples(cold_only=True) or the saved folders" % self.dist.get_world_size())
        from .diagnostics import diagnose, ladder_index
        d = self.samples_dev(phase)
        T = int(d["likes"].shape[0])
        if not T:
            raise EngineError("ladder_diagnostics(): no snapshot of phase %r yet" % (phase,))
        with self.torch.cuda.device(self.dev):
            idx = ladder_index(d["beta"], self.ladder, engine=self.engine)
            ids = np.asarray(idx["ids"], dtype=np.int64)
            site_of_ladder = np.array([m[0] // self.C_site for m in idx["members"]], dtype=np.int64)
            r = diagnose(d, site_of_ladder, ids, dev=dev, dep=dep, maxlag=maxlag, exclude_chains=exclude_ladders, engine=self.engine,
                         sel=idx["sel"], features=features, moho=moho, mohovs=mohovs)
        pos = {int(l): k for k, l in enumerate(ids)}
        for s, rs in enumerate(r):
            ks = np.flatnonzero(site_of_ladder == s)
            members = [self.chain_offset + idx["members"][k].astype(np.int64) for k in ks]
            local = np.sort(np.concatenate([idx["members"][k] for k in ks]))      # the site's chains, in chain order
            occ = idx["occupancy"][local]
            rs["outlier_chains"] = (np.concatenate([self.chain_offset + idx["members"][pos[int(l)]].astype(np.int64) for l in rs["outliers"]])
                                    if len(rs["outliers"]) else np.zeros(0, np.int64))
            rs["ladders"] = dict(ids=ids[ks], members=members, moves=idx["moves"][ks], chains=self.chain_offset + local.astype(np.int64),
                                 round_trips=idx["round_trips"][local], occupancy=occ, cold_share=occ[:, 0] / float(T))
        return r if self.sites is not None else r[0]

    def ladder_evidence(self, phase="p2", maxlag=None):
        """record="device", tempered runs: the log-evidence of every site's ladders from the recorded rungs, straight from the
        device store -- diagnostics.ladder_evidence on samples_dev(phase)'s likes and beta where they lie.  The hot rungs, which
        the posterior methods leave out, are exactly the samples the marginal likelihood is estimated from: stepping stones in
        both directions (`ss`, biased low, and `ss_rev`, biased high) and thermodynamic integration (`ti`, `ti2`), each
        log Z(b_0) - log Z(b_min) of a ladder, Z(b) the integral of prior x L^b over the transdimensional prior -- the evidence
        proper only for a ladder from beta = 1 down to beta = 0 (`complete`).  One dict per site (one dict without SiteTargets):
        `ids` (the site's ladder ids), `members` (global chain numbers per ladder), `ladders` (per ladder the dict of
        diagnostics.ladder_evidence: betas, mean, var, tau, ess, rhat, log_ratio, log_ratio_rev, ss, ss_err, ss_rev, ss_rev_err,
        ti, ti2, ti_err, beta_min, complete), `logz` = the mean of `ss` over the site's ladders and `logz_spread` = their standard
        deviation (ddof 1; NaN for one ladder): replicate ladders are the honest error bar, the per-ladder errors take the rung
        series' ESS for a number of independent terms.  Saved folders hold the cold samples only: nothing of this is read from them.
        EngineError: record="host", an untempered run, a sharded job of more than one rank (ladders are not followed across
        ranks); and from the engine a phase in which ladder_adapt moved the betas ("change within the rows": the burn-in of an
        adapting run -- the main phase holds them)."""
        if self._rec is None:
            raise EngineError("ladder_evidence() needs DeviceChains(record='device'): record='host' keeps no time-ordered store of "
                              "the chains on the GPU, and saved folders hold the cold samples only")
        if self.t["beta"] is None or self.ladder is None:
            raise EngineError("ladder_evidence() of an untempered run: there are no ladders, and one temperature holds no evidence "
                              "estimate")
        if self.dist is not None and self.dist.is_initialized() and self.dist.get_world_size() > 1:
            raise EngineError("ladder_evidence() does not follow ladders across ranks (world size %d)" % self.dist.get_world_size())
        from .diagnostics import ladder_evidence
        d = self.samples_dev(phase)
        if not int(d["likes"].shape[0]):
            raise EngineError("ladder_evidence(): no snapshot of phase %r yet" % (phase,))
        with self.torch.cuda.device(self.dev):
            ev = ladder_evidence(d["beta"], d["likes"], self.ladder, maxlag=maxlag, engine=self.engine)
        ids = np.asarray(ev["ids"], dtype=np.int64)
        site_of_ladder = np.array([m[0] // self.C_site for m in ev["members"]], dtype=np.int64)
        out = []
        for s in range(self.nsites):
            ks = np.flatnonzero(site_of_ladder == s)
            ss = np.array([ev["ladders"][k]["ss"] for k in ks], dtype=np.float64)
            out.append(dict(ids=ids[ks], members=[self.chain_offset + ev["members"][k].astype(np.int64) for k in ks],
                            ladders=[ev["ladders"][k] for k in ks], logz=float(np.mean(ss)) if ss.size else float("nan"),
                            logz_spread=float(np.std(ss, ddof=1)) if ss.size > 1 else float("nan")))
        return out if self.sites is not None else out[0]

    def _host_rows(self, phase):
        """the rows of samples() from the host snapshots of run()"""
        S = self.snap[phase]
        ns, Cn, ML = len(S), self.C, self.ML
        models = np.full((ns, Cn, 2 * ML), np.nan, dtype=np.float32)
        j = np.arange(2 * ML)[:, None]                               # position inside a reference row
        for i, r in enumerate(S):
            n = r["n"][None, :].astype(np.int64)                      # [1, C]
            # reference rows hold the n vs values first, then the n depths, then NaN padding
            both = np.vstack((r["vs"], r["z"]))                       # [2*ML, C]: vs rows, then z rows
            src = np.where(j < n, j, ML + (j - n))                    # row of `both` feeding position j
            row = np.take_along_axis(both, np.clip(src, 0, 2 * ML - 1), axis=0)
            models[i] = np.where(j < 2 * n, row, np.nan).T
        out = dict(models=models)
        for k in ("like", "vpvs"):
            out[k + "s" if k == "like" else k] = np.array([r[k] for r in S], dtype=np.float32).reshape(ns, Cn)
        out["misfits"] = np.array([r["misfits"].T for r in S], dtype=np.float32).reshape(ns, Cn, self.nt + 1)
        out["noise"] = np.array([r["noise"].T for r in S], dtype=np.float32).reshape(ns, Cn, 2 * self.nt)
        if ns and S[0]["beta"] is not None:
            out["beta"] = np.array([r["beta"] for r in S]).reshape(ns, Cn)   # cold samples: out["beta"] == 1
        return out

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
