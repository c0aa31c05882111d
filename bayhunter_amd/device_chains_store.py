"""The device record of `DeviceChains(record="device")` and what reads it: the store the accept kernel writes the thinned rows
into (include/bh_engine_chain_record.h), its views (`samples_dev`), the posterior summaries of the rows where they lie
(`posterior_*`) and the convergence diagnostics of the recorded series (`diagnostics`, `ladder_diagnostics`, `ladder_evidence`).
`ChainStore` is mixed into `DeviceChains` (bayhunter_amd/device_chains.py), which runs the chains; nothing here advances them."""
import numpy as np

from .engine import ChainRecord, EngineError


class ChainStore(object):
    """The methods of DeviceChains over its device store.  Reads of the run: C, C_site, ML, nt, nsites, sites, targets, site_priors,
    ladder, chain_offset, dist, t, dev, engine, torch, iiter, iter_phase1, iter_phase2, thinning, initparams; owns store / _rec."""

    def _allocate_store(self, tempered):
        """the device store of record="device": every row of both phases (include/bh_engine_chain_record.h)"""
        from .device_chains import record_rows
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

    def _store_range(self, phase):
        """rows [lo, hi) of the device store that hold the snapshots of `phase` taken so far (up to the current iiter)"""
        from .device_chains import record_rows, snapshot_count
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

    def _need_store(self, what, tempered=None, one_rank=None):
        """The refusals of the methods that read the device store, in their order, each with its caller's text: `what` without a
        store (record="host"); tempered = (the kind of run the caller needs, its text otherwise); one_rank = its text (% the world
        size) for a sharded job of more than one rank.  None: not checked."""
        if self._rec is None:
            raise EngineError(what)
        if tempered is not None and (self.t["beta"] is not None) != tempered[0]:
            raise EngineError(tempered[1])
        if one_rank is not None and self.dist is not None and self.dist.is_initialized() and self.dist.get_world_size() > 1:
            raise EngineError(one_rank % self.dist.get_world_size())

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
        self._need_store("samples_dev() needs DeviceChains(record='device')")
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

    # ---- the posterior_* methods: one frame, and the pieces several of them share ------------------------------------
    def _selection(self, phase, cold_only, exclude_chains):
        """(phase, cold_only, exclude_chains) as posterior_classes() remembers it: cold_only None = True on tempered runs"""
        if cold_only is None:
            cold_only = self.ladder is not None
        return (phase, bool(cold_only), tuple(int(c) for c in np.atleast_1d(np.asarray(exclude_chains, dtype=np.int64))))

    def _on_rows(self, body, phase, cold_only, exclude_chains, classes=None, per_site=True):
        """The frame of every posterior_* method: classes= must stem from the same selection of the store's rows; body(d, n, kw)
        runs on the chains' GPU with d = samples_dev() of the selection, n = its rows and kw = the site and engine arguments of
        the posterior functions; per_site: a list of one result per site comes back as its only entry without SiteTargets."""
        sel = self._selection(phase, cold_only, exclude_chains)
        if classes is not None:
            if not isinstance(classes, dict) or "selection" not in classes:
                raise ValueError("classes must be the dict DeviceChains.posterior_classes returned")
            if tuple(classes["selection"]) != sel:
                raise ValueError("classes was formed with (phase, cold_only, exclude_chains) = %r, this call asks for %r: classify "
                                 "the same rows" % (tuple(classes["selection"]), sel))
        d = self.samples_dev(phase, cold_only=sel[1], exclude_chains=exclude_chains)
        with self.torch.cuda.device(self.dev):
            r = body(d, d["models2d"].shape[0], dict(site=d["site"], engine=self.engine))
        return r if self.sites is not None or not per_site else r[0]

    def _store_columns(self, d, names, allow_nlayers):
        """(names as a tuple, name -> the store's column over the rows of d) for scalars= of the posterior_* methods; "nlayers",
        where allowed, is no column of the store and gets none.  ValueError: any other name."""
        n = d["models2d"].shape[0]
        shapes = dict(likes=(n,), vpvs=(n,), misfits=(n, self.nt + 1), noise=(n, 2 * self.nt))
        if isinstance(names, str):
            names = (names,)
        unknown = [k for k in names if k not in shapes and not (allow_nlayers and k == "nlayers")]
        if unknown:
            raise ValueError("scalars: %r is no column of the store (%s%s)" % (unknown[0], ", ".join(shapes), ", nlayers" if allow_nlayers else ""))
        return names, {k: d[k].reshape(shapes[k]) for k in names if k != "nlayers"}

    def _site_z(self):
        """every site's own priors['z']: what moho=True (posterior_moho: None) stands for"""
        return [tuple(float(v) for v in p["z"]) for p in self.site_priors]

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

        def body(d, n, kw):
            names, cols = self._store_columns(d, scalars, True)
            return posterior_classes(d["models2d"], classes, features=features, moho=self._site_z() if moho is True else moho,
                                     mohovs=mohovs, columns=cols or None, nlayers="nlayers" in names, nsites=self.nsites, **kw)
        r = self._on_rows(body, phase, cold_only, exclude_chains, per_site=False)
        r["selection"] = self._selection(phase, cold_only, exclude_chains)
        return r

    def posterior_models(self, dep_int=None, quantiles=None, phase="p2", cold_only=None, exclude_chains=(), classes=None):
        """record="device": bayhunter_amd.posterior_models of every site's recorded rows, straight from the device store (one dict
        per site; one dict without SiteTargets): mean, median, minmax, stdminmax, mode and -- the joint misfit misfits[..., -1]
        being in the store -- minmisfit of vs against depth; quantiles (numbers in [0, 1]) adds the credible band `quantiles`.
        cold_only (default: True on tempered runs) and exclude_chains as in samples_dev().  classes: the dict
        posterior_classes() returned for the same phase, cold_only and exclude_chains: per site a dict class name -> that dict."""
        from .posterior import posterior_models
        return self._on_rows(lambda d, n, kw: posterior_models(d["models2d"], dep_int=dep_int, misfits=d["misfits"][..., -1].reshape(n),
                                                               nsites=self.nsites, quantiles=quantiles, classes=classes, **kw),
                             phase, cold_only, exclude_chains, classes)

    def posterior_hist2d(self, dep_int=None, vs_edges=None, dep_edges=None, phase="p2", cold_only=None, exclude_chains=(), classes=None):
        """record="device": bayhunter_amd.posterior_hist2d of every site's recorded rows, straight from the device store (one dict
        per site; one dict without SiteTargets): the 2-D posterior plot's vs-depth histogram and the histogram of interface
        depths.  cold_only (default: True on tempered runs) and exclude_chains as in samples_dev().  classes: the dict
        posterior_classes() returned for the same phase, cold_only and exclude_chains: per site a dict class name -> that dict."""
        from .posterior import posterior_hist2d
        return self._on_rows(lambda d, n, kw: posterior_hist2d(d["models2d"], dep_int=dep_int, vs_edges=vs_edges, dep_edges=dep_edges,
                                                               nsites=self.nsites, classes=classes, **kw),
                             phase, cold_only, exclude_chains, classes)

    def posterior_moho(self, moho=None, mohovs=4.2, bins=50, phase="p2", cold_only=None, exclude_chains=(), quantiles=None, classes=None):
        """record="device": bayhunter_amd.posterior_moho of every site's recorded rows, straight from the device store (one dict
        per site; one dict without SiteTargets).  moho None: every site's own priors['z'], the reference's default.  cold_only
        (default: True on tempered runs) and exclude_chains as in samples_dev().  quantiles: as posterior_moho's.  classes: the dict
        posterior_classes() returned for the same phase, cold_only and exclude_chains: per site a dict class name -> that dict."""
        from .posterior import posterior_moho
        return self._on_rows(lambda d, n, kw: posterior_moho(d["models2d"], moho=self._site_z() if moho is None else moho, mohovs=mohovs,
                                                             bins=bins, nsites=self.nsites, quantiles=quantiles, classes=classes, **kw),
                             phase, cold_only, exclude_chains, classes)

    def posterior_features(self, features, bins=50, phase="p2", cold_only=None, exclude_chains=(), quantiles=None, classes=None):
        """record="device": bayhunter_amd.posterior_features of every site's recorded rows, straight from the device store (one dict
        per site; one dict without SiteTargets): the posteriors of structural features of the layered models -- features: name ->
        (kind, z0, z1[, c]), every number one value or one per site.  cold_only (default: True on tempered runs) and
        exclude_chains as in samples_dev().  quantiles: as posterior_features'.  classes: the dict
        posterior_classes() returned for the same phase, cold_only and exclude_chains: per site a dict class name -> that dict."""
        from .posterior import posterior_features
        return self._on_rows(lambda d, n, kw: posterior_features(d["models2d"], features, bins=bins, quantiles=quantiles,
                                                                 nsites=self.nsites, classes=classes, **kw),
                             phase, cold_only, exclude_chains, classes)

    def posterior_scalars(self, bins=20, nlayers=True, phase="p2", cold_only=None, exclude_chains=(), quantiles=None, classes=None):
        """record="device": bayhunter_amd.posterior_scalars of every site's recorded rows with the store's likes, vpvs, misfits
        [nt+1] and noise [2nt] as columns (slot layout), straight from the device store (one dict per site; one dict without
        SiteTargets).  cold_only (default: True on tempered runs) and exclude_chains as in samples_dev().  quantiles: as
        posterior_scalars'.  classes: the dict
        posterior_classes() returned for the same phase, cold_only and exclude_chains: per site a dict class name -> that dict."""
        from .posterior import posterior_scalars
        return self._on_rows(lambda d, n, kw: posterior_scalars(d["models2d"], self._store_columns(d, ("likes", "vpvs", "misfits", "noise"), False)[1],
                                                                bins=bins, nlayers=nlayers, nsites=self.nsites, quantiles=quantiles,
                                                                classes=classes, **kw),
                             phase, cold_only, exclude_chains, classes)

    def posterior_covariance(self, dep_int=None, scalars=(), moho=None, mohovs=4.2, phase="p2", cold_only=None, exclude_chains=(),
                             features=None, classes=None):
        """record="device": bayhunter_amd.posterior_covariance of every site's recorded rows, straight from the device store (one
        dict per site; one dict without SiteTargets): mean, covariance and correlation of vs at the depths of dep_int.  scalars:
        names of the store's columns to put beside the depths -- likes, vpvs, misfits [nt+1] and noise [2nt], as
        posterior_scalars() takes them; or moho = (lo, hi) (True: every site's own priors['z']) with mohovs for the Moho depth and
        the mean crustal vs; or features: name -> (kind, z0, z1[, c]) as posterior_features() takes them -- one of the three.  cold_only
        (default: True on tempered runs) and exclude_chains as in samples_dev().  classes: the dict
        posterior_classes() returned for the same phase, cold_only and exclude_chains: per site a dict class name -> that dict."""
        from .posterior import posterior_covariance
        return self._on_rows(lambda d, n, kw: posterior_covariance(d["models2d"], dep_int=dep_int, columns=self._store_columns(d, scalars, False)[1] or None,
                                                                   moho=self._site_z() if moho is True else moho, mohovs=mohovs,
                                                                   nsites=self.nsites, features=features, classes=classes, **kw),
                             phase, cold_only, exclude_chains, classes)

    def posterior_datafits(self, quantiles=(0.025, 0.16, 0.5, 0.84, 0.975), phase="p2", cold_only=None, exclude_chains=()):
        """record="device": bayhunter_amd.posterior_datafits of every site's recorded rows, straight from the device store (one
        dict per site; one dict without SiteTargets): the best fit of every chain -- the chain id is the row's column in the
        store, misfits[..., -1] the joint misfit -- and the predictive band of every datum; every site's mantle rule is that of
        its priors.  cold_only (default: True on tempered runs) and exclude_chains as in samples_dev()."""
        from .datafits import posterior_datafits

        def body(d, n, kw):
            chain = self.torch.arange(self.C, dtype=self.torch.int32, device=self.dev).repeat(n // self.C if self.C else 0)
            return posterior_datafits(self.sites if self.sites is not None else self.targets, d["models2d"], d["vpvs"].reshape(n),
                                      chain=chain, misfits=d["misfits"][..., -1].reshape(n), quantiles=quantiles,
                                      mantle=[p.get("mantle") for p in self.site_priors], **kw)
        return self._on_rows(body, phase, cold_only, exclude_chains, per_site=False)

    def posterior_residuals(self, maxlag=10, quantiles=(0.025, 0.16, 0.5, 0.84, 0.975), phase="p2", cold_only=None, exclude_chains=()):
        """record="device": bayhunter_amd.posterior_residuals of every site's recorded rows, straight from the device store (one
        dict per site; one dict without SiteTargets): whether the residuals of the recorded models look like the noise each row
        assumed -- the store's noise table [2nt] (slot layout) is read where it lies; every site's mantle rule is that of its
        priors.  cold_only (default: True on tempered runs) and exclude_chains as in samples_dev()."""
        from .datafits import posterior_residuals
        return self._on_rows(lambda d, n, kw: posterior_residuals(self.sites if self.sites is not None else self.targets, d["models2d"],
                                                                  d["vpvs"].reshape(n), d["noise"].reshape(n, 2 * self.nt), maxlag=maxlag,
                                                                  quantiles=quantiles, mantle=[p.get("mantle") for p in self.site_priors], **kw),
                             phase, cold_only, exclude_chains, per_site=False)

    # ---- convergence of the recorded series ---------------------------------------------------------------------------
    def _site_ladders(self, members):
        """From the members of every ladder (chain positions on this rank, one array per ladder): the site of every ladder, and per
        site (the positions of its ladders in `members`, their members' global chain numbers)."""
        site_of = np.array([m[0] // self.C_site for m in members], dtype=np.int64)
        return site_of, [(ks, [self.chain_offset + members[k].astype(np.int64) for k in ks])
                         for ks in (np.flatnonzero(site_of == s) for s in range(self.nsites))]

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
        self._need_store("diagnostics() needs DeviceChains(record='device'): record='host' keeps no time-ordered store of the "
                         "chains on the GPU (results.diagnostics_from_storage reads saved folders)",
                         (False, "diagnostics() of a tempered run: a ladder's cold state moves between chains, so no chain's recorded "
                                 "series is a series of posterior samples"),
                         "diagnostics() of a sharded job (world size %d): the chains of a site lie on several ranks")
        from .diagnostics import diagnose
        d = self.samples_dev(phase)
        if not d["likes"].shape[0]:
            raise EngineError("diagnostics(): no snapshot of phase %r yet" % (phase,))
        with self.torch.cuda.device(self.dev):
            r = diagnose(d, np.arange(self.C) // self.C_site, self.chain_offset + np.arange(self.C, dtype=np.int64), dev=dev, dep=dep, maxlag=maxlag, exclude_chains=exclude_chains,
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
        self._need_store("ladder_diagnostics() needs DeviceChains(record='device'): record='host' keeps no time-ordered store of "
                         "the chains on the GPU (results.diagnostics_from_storage reads saved folders)",
                         (True, "ladder_diagnostics() of an untempered run: there are no ladders -- every chain's own series is a "
                                "posterior series, use diagnostics()"),
                         "ladder_diagnostics() does not follow ladders across ranks (world size %d): use "
                         "samples(cold_only=True) or the saved folders")
        from .diagnostics import diagnose, ladder_index
        d = self.samples_dev(phase)
        T = int(d["likes"].shape[0])
        if not T:
            raise EngineError("ladder_diagnostics(): no snapshot of phase %r yet" % (phase,))
        with self.torch.cuda.device(self.dev):
            idx = ladder_index(d["beta"], self.ladder, engine=self.engine)
            ids = np.asarray(idx["ids"], dtype=np.int64)
            site_of_ladder, per_site = self._site_ladders(idx["members"])
            r = diagnose(d, site_of_ladder, ids, dev=dev, dep=dep, maxlag=maxlag, exclude_chains=exclude_ladders, engine=self.engine,
                         sel=idx["sel"], features=features, moho=moho, mohovs=mohovs)
        pos = {int(l): k for k, l in enumerate(ids)}
        for rs, (ks, members) in zip(r, per_site):
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
        self._need_store("ladder_evidence() needs DeviceChains(record='device'): record='host' keeps no time-ordered store of "
                         "the chains on the GPU, and saved folders hold the cold samples only",
                         (True, "ladder_evidence() of an untempered run: there are no ladders, and one temperature holds no evidence "
                                "estimate"),
                         "ladder_evidence() does not follow ladders across ranks (world size %d)")
        from .diagnostics import ladder_evidence
        d = self.samples_dev(phase)
        if not int(d["likes"].shape[0]):
            raise EngineError("ladder_evidence(): no snapshot of phase %r yet" % (phase,))
        with self.torch.cuda.device(self.dev):
            ev = ladder_evidence(d["beta"], d["likes"], self.ladder, maxlag=maxlag, engine=self.engine)
        ids = np.asarray(ev["ids"], dtype=np.int64)
        out = []
        for ks, members in self._site_ladders(ev["members"])[1]:
            ss = np.array([ev["ladders"][k]["ss"] for k in ks], dtype=np.float64)
            out.append(dict(ids=ids[ks], members=members, ladders=[ev["ladders"][k] for k in ks],
                            logz=float(np.mean(ss)) if ss.size else float("nan"),
                            logz_spread=float(np.std(ss, ddof=1)) if ss.size > 1 else float("nan")))
        return out if self.sites is not None else out[0]
