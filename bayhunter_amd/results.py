"""Result store of an inversion in the reference's on-disk format, so that the reference's
`PlotFromStorage(configfile)` opens a folder written by this package:

    <savepath>/data/<station>_config.pkl      save_config          (src/utils.py:127-153, src/mcmcOptimizer.py:52-55)
    <savepath>/data/c%03d_p{1,2}*.npy         ChainBatch.save / DeviceChains.save  (src/SingleChain.py:646-690)
    <savepath>/data/outliers.dat              get_outliers         (src/Plotting.py:113-151)
    <savepath>/data/c_{models,likes,misfits,noise,vpvs}.npy   save_final_distribution (src/Plotting.py:157-262)

Host I/O only -- nothing here touches the GPU.
"""
import glob
import os
import os.path as op
import pickle
import sys

import numpy as np

# the reference's class of every object inside a pickled target (module path in the reference package)
_REF_CLASS = {
    "RayleighDispersionPhase": "BayHunter.Targets", "RayleighDispersionGroup": "BayHunter.Targets",
    "LoveDispersionPhase": "BayHunter.Targets", "LoveDispersionGroup": "BayHunter.Targets",
    "PReceiverFunction": "BayHunter.Targets", "SReceiverFunction": "BayHunter.Targets",
    "SingleTarget": "BayHunter.Targets", "ObservedData": "BayHunter.Targets", "ModeledData": "BayHunter.Targets",
    "Valuation": "BayHunter.Targets", "SurfDisp": "BayHunter.surf96_modsw", "RFminiModRF": "BayHunter.rfmini_modrf",
}
_RF_KEYS = {"z": "%.2f", "vp": "%.4f", "vs": "%.4f", "rho": "%.4f", "qp": "%.1f", "qs": "%.1f", "n": "%d"}


def _shadow(obj, classes):
    """A copy of `obj` as an instance of the reference's class of the same name (state = the attributes the
    reference's object holds: this package's classes mirror them; engine handles and bound methods are dropped)."""
    name = type(obj).__name__
    if name not in _REF_CLASS:
        return obj
    state = {}
    for k, v in obj.__dict__.items():
        if k.startswith("_") or k in ("noise_law", "get_covariance"):
            continue
        state[k] = _shadow(v, classes) if type(v).__name__ in _REF_CLASS else v
    if name in ("SingleTarget",) or _REF_CLASS[name] == "BayHunter.Targets" and "obsdata" in state:
        state["get_covariance"] = None       # the reference resets the bound method before pickling (utils.py:142-143)
    if name == "RFminiModRF":
        state.setdefault("keys", dict(_RF_KEYS))
    inst = object.__new__(classes[name])
    inst.__dict__.update(state)
    return inst


def _reference_classes():
    """name -> class object standing for the reference's class of that name while pickling.  Where the reference
    package itself is already imported its own classes are used; otherwise empty stand-in classes that carry the
    reference's (module, name) -- `_RefPickler` writes that name into the file (pickle stores classes BY NAME: the
    file then loads into the real classes wherever the reference is installed).  Nothing is registered in
    sys.modules: a concurrent `import BayHunter` in another thread never sees a stand-in."""
    classes = {}
    for name, mod in _REF_CLASS.items():
        m = sys.modules.get(mod)
        if m is not None and hasattr(m, name):
            classes[name] = getattr(m, name)
        else:
            classes[name] = type(name, (object,), {"__module__": mod, "_bh_ref_path": (mod, name)})
    return classes


class _RefPickler(pickle._Pickler):
    """The pure-Python pickler with one change: a stand-in class is written as the GLOBAL it stands for, without the
    importability check of `save_global` (the class lives in the reference package, which need not be installed
    where the file is written).  The dispatch table is this class's own copy with its own handler for classes:
    libraries that extend the stock table process-wide (dill does, once imported) do not change what is written."""
    dispatch = dict(pickle._Pickler.dispatch)

    def _save_class(self, obj):
        ref = obj.__dict__.get("_bh_ref_path")
        if ref is None:
            return pickle._Pickler.save_global(self, obj)
        self.write(pickle.GLOBAL + ref[0].encode("ascii") + b"\n" + ref[1].encode("ascii") + b"\n")
        self.memoize(obj)

    dispatch[type] = _save_class


def save_config(targets, configfile, priors=None, initparams=None):
    """Write the configuration pickle `PlotFromStorage.__init__` needs (src/Plotting.py:52-58): the targets (as
    instances of the reference's classes), their refs, priors and initparams (src/utils.py:127-153)."""
    tl = targets.targets if hasattr(targets, "targets") else list(targets)
    classes = _reference_classes()
    data = {"targets": [_shadow(t, classes) for t in tl], "targetrefs": [t.ref for t in tl],
            "priors": dict(priors or {}), "initparams": dict(initparams or {})}
    os.makedirs(op.dirname(op.abspath(configfile)), exist_ok=True)
    with open(configfile, "wb") as f:
        _RefPickler(f, protocol=2).dump(data)
    return configfile


def _chainfiles(datapath, phase, ftype):
    return sorted(glob.glob(op.join(datapath, "c???_p%d%s.npy" % (phase, ftype))))


def _chainidx(path):
    return int(op.basename(path)[1:4])


def get_outliers(datapath, dev=0.05):
    """Outlier chains by the median likelihood of the main phase relative to the best chain
    (src/Plotting.py:113-151); writes outliers.dat when there are any."""
    likefiles = _chainfiles(datapath, 2, "likes")
    chainidxs = np.array([_chainidx(f) for f in likefiles], dtype=float)
    chainmedians = np.array([np.median(np.load(f)) for f in likefiles])
    maxlike = np.max(chainmedians)
    if maxlike > 0:
        scores = chainmedians / maxlike
    elif maxlike < 0:
        scores = maxlike / chainmedians
    else:
        scores = np.ones_like(chainmedians)
    sel = np.where((1 - scores) > dev)
    outliers, outscores = chainidxs[sel], 1 - scores[sel]
    if len(outliers) > 0:
        with open(op.join(datapath, "outliers.dat"), "w") as f:
            f.write("# Outlier chainindices with %.3f deviation condition\n" % dev)
            for i, o in enumerate(outliers):
                f.write("%d\t%.3f\n" % (o, outscores[i]))
    return outliers


def save_final_distribution(datapath, maxmodels=200000, dev=0.05, rstate=None):
    """Merge the main-phase files of all non-outlier chains into c_{models,likes,misfits,noise,vpvs}.npy, the same
    number of models from every chain (src/Plotting.py:157-262).  `rstate`: the generator the reference's
    Plotting module draws the per-chain subsets from -- a module-level RandomState(333); a fresh one per call here,
    i.e. the files equal those of the reference's FIRST call in a process."""
    rstate = np.random.RandomState(333) if rstate is None else rstate
    outlierfile = op.join(datapath, "outliers.dat")
    if op.exists(outlierfile):
        os.remove(outlierfile)
    outliers = get_outliers(datapath, dev=dev)
    files = {k: _chainfiles(datapath, 2, k) for k in ("models", "likes", "misfits", "noise", "vpvs")}
    nchains = int(len(files["likes"]) - outliers.size)
    maxmodels = int(maxmodels)
    mpc = int(maxmodels / nchains)
    out = {k: None for k in files}
    alllikes = np.ones(maxmodels) * np.nan
    start = 0
    for i, lf in enumerate(files["likes"]):
        if _chainidx(lf) in outliers:
            continue
        n = len(np.load(lf))
        index = np.arange(n).astype(int)
        if n > mpc:
            index = rstate.choice(index, mpc, replace=False)
            index.sort()
        end = start + index.size
        for k in files:
            data = np.load(files[k][i])[index]
            if k == "likes":
                alllikes[start:end] = data
                continue
            if out[k] is None:
                out[k] = np.ones((maxmodels,) + data.shape[1:]) * np.nan
            out[k][start:end] = data
        start = end
    keep = ~np.isnan(alllikes)
    out["likes"] = alllikes
    for k in ("models", "likes", "misfits", "noise", "vpvs"):
        np.save(op.join(datapath, "c_%s" % k), out[k][keep])
    return outliers


def posterior_from_storage(datapaths, dep_int=None, engine=None, quantiles=None):
    """Posterior velocity-depth summaries of many sites in one GPU call (bayhunter_amd.posterior.posterior_models):
    datapaths[s] is site s's data directory after save_final_distribution (c_models.npy; c_misfits.npy, its last column
    the joint misfit, for `minmisfit`).  Rows of different widths are padded with NaN.  quantiles: as posterior_models' (the
    credible band of vs against depth).  Returns one dict per site."""
    from .posterior import posterior_models
    models = [np.load(op.join(p, "c_models.npy")) for p in datapaths]
    misfits = []
    for p, m in zip(datapaths, models):
        f = op.join(p, "c_misfits.npy")
        misfits.append(np.load(f).reshape(len(m), -1)[:, -1] if op.exists(f) else None)
    W = max(m.shape[1] for m in models)
    rows = np.full((sum(len(m) for m in models), W), np.nan)
    site = np.zeros(len(rows), np.int32)
    start = 0
    for s, m in enumerate(models):
        rows[start:start + len(m), :m.shape[1]] = m
        site[start:start + len(m)] = s
        start += len(m)
    mis = None if any(x is None for x in misfits) else np.concatenate(misfits)
    return posterior_models(rows, site=site, dep_int=dep_int, misfits=mis, engine=engine, nsites=len(datapaths),
                            quantiles=quantiles)


def _site_features(features, moho, mohovs, S, s):
    """features, moho, mohovs of site s of S: a number given per site takes the site's position"""
    from .posterior import _per_site, check_features
    if features is not None:
        check_features(features, S)
        features = {name: (spec[0],) + tuple(float(np.broadcast_to(np.asarray(v, np.float64), (S,))[s]) for v in spec[1:])
                    for name, spec in features.items()}
    if moho is not None:
        moho, mohovs = tuple(_per_site(moho, S, 2, "moho")[s]), float(_per_site(mohovs, S, 0, "mohovs")[s])
    return features, moho, mohovs


def diagnostics_from_storage(datapaths, dep=None, maxlag=None, dev=0.05, exclude_chains=None, engine=None, rank=False, features=None,
                             moho=None, mohovs=4.2):
    """Outlier chains, split R-hat and effective sample sizes of many sites from saved folders (bayhunter_amd.diagnostics, what
    DeviceChains.diagnostics gives from the device store): datapaths[s] is site s's data directory; its main-phase chain files
    c???_p2{likes,vpvs,misfits,noise,models}.npy -- per chain and time-ordered -- are stacked to [T][C][..] tables and go through
    the same calls.  `outliers` and `exclude_chains` (None: the outliers; else one sequence for all sites) are file numbers.
    rank=True: every group's dict gains "rank", the rank-normalised R-hat and the bulk and tail ESS (diagnostics.rank_convergence).
    features, moho, mohovs: as DeviceChains.diagnostics -- every site's dict gains "features" (diagnostics.feature_convergence);
    one folder is one site, and a number given per site takes the folder's position.
    ValueError: chains of unequal length.  Returns one dict per site."""
    from .diagnostics import diagnose, stack_chain_files
    out = []
    for s, p in enumerate(datapaths):
        tabs, ids = stack_chain_files(p)
        ex = None if exclude_chains is None else [c for c in np.atleast_1d(exclude_chains) if c in ids]
        ft, mo, mv = _site_features(features, moho, mohovs, len(datapaths), s)
        out.append(diagnose(tabs, np.zeros(ids.size, np.int64), ids, dev=dev, dep=dep, maxlag=maxlag, exclude_chains=ex,
                            engine=engine, rank=rank, features=ft, moho=mo, mohovs=mv)[0])
    return out


class _PriorsUnpickler(pickle.Unpickler):
    """Reads <station>_config.pkl where the reference is not installed: a class that cannot be imported (the reference's
    targets) becomes an empty stand-in -- only the plain dicts of the file are used."""

    def find_class(self, module, name):
        try:
            return pickle.Unpickler.find_class(self, module, name)
        except (ImportError, AttributeError):
            return type(str(name), (object,), {})


def _saved_config(datapath):
    files = sorted(glob.glob(op.join(datapath, "*_config.pkl")))
    if len(files) != 1:
        raise IOError("%s: expected one *_config.pkl, found %d" % (datapath, len(files)))
    with open(files[0], "rb") as f:
        return _PriorsUnpickler(f).load()


def saved_priors(datapath):
    """The `priors` dict of the one *_config.pkl in a station's data folder (save_config)."""
    return _saved_config(datapath)["priors"]


def saved_targets(datapath):
    """The targets of a station's *_config.pkl as this package's own targets: x, y, yerr, the plugin's parameters and the
    mode / flsph are taken over from the saved objects (read without the reference installed).  The file does not say which noise
    law the sampler installed: the targets get 'nocorr', which is enough for their forward models."""
    from . import Targets as T
    out = []
    for t in _saved_config(datapath)["targets"]:
        cls = getattr(T, type(t).__name__)
        o = t.obsdata
        new = cls(np.asarray(o.x, dtype=float), np.asarray(o.y, dtype=float), yerr=getattr(o, "yerr", None))
        plug = getattr(getattr(t, "moddata", None), "plugin", None)
        params = getattr(plug, "modelparams", None)
        if params:
            new.moddata.plugin.set_modelparams(**dict(params))
        new.set_noise_law("nocorr")
        out.append(new)
    return out


def _stack_sites(arrays):
    """rows of many sites under each other, padded with NaN to the widest, and every row's site index"""
    W = max(a.shape[1] for a in arrays)
    rows = np.full((sum(len(a) for a in arrays), W), np.nan)
    site = np.zeros(len(rows), np.int32)
    start = 0
    for s, a in enumerate(arrays):
        rows[start:start + len(a), :a.shape[1]] = a
        site[start:start + len(a)] = s
        start += len(a)
    return rows, site


def moho_from_storage(datapaths, moho=None, mohovs=4.2, bins=50, engine=None, quantiles=None):
    """Moho depth and crustal velocity posteriors of many sites in one GPU call (bayhunter_amd.posterior.posterior_moho, the
    numbers of the reference's plot_moho_crustvel_tradeoff): datapaths[s] is site s's data directory after
    save_final_distribution (c_models.npy).  moho: (lo, hi) km, one pair per site, or None -- then every site's range is its
    saved priors['z'] (<station>_config.pkl in the same folder), the reference's default.  quantiles: as posterior_moho's (the
    credible interval of the Moho depth).  Returns one dict per site."""
    from .posterior import posterior_moho
    if moho is None:
        moho = [tuple(float(v) for v in saved_priors(p)["z"]) for p in datapaths]
    rows, site = _stack_sites([np.load(op.join(p, "c_models.npy")) for p in datapaths])
    return posterior_moho(rows, site=site, moho=moho, mohovs=mohovs, bins=bins, engine=engine, nsites=len(datapaths),
                          quantiles=quantiles)


def features_from_storage(datapaths, features, bins=50, engine=None, quantiles=None):
    """Posteriors of structural features of the layered models of many sites in one GPU call
    (bayhunter_amd.posterior.posterior_features): datapaths[s] is site s's data directory after save_final_distribution
    (c_models.npy).  features: name -> (kind, z0, z1[, c]), every number one value or one per site; bins and quantiles as
    posterior_features'.  Returns one dict per site."""
    from .posterior import posterior_features
    rows, site = _stack_sites([np.load(op.join(p, "c_models.npy")) for p in datapaths])
    return posterior_features(rows, features, site=site, bins=bins, quantiles=quantiles, engine=engine, nsites=len(datapaths))


def covariance_from_storage(datapaths, dep_int=None, moho=None, mohovs=4.2, engine=None):
    """Mean, covariance and correlation of vs with depth of many sites in one GPU call (bayhunter_amd.posterior.posterior_covariance):
    datapaths[s] is site s's data directory after save_final_distribution (c_models.npy).  moho: None -- the vs at the depths of
    dep_int alone; (lo, hi) km or one pair per site, or True for every site's saved priors['z'] -- the Moho depth and the mean
    crustal vs are appended (rows without a Moho are then left out of the matrix).  Returns one dict per site."""
    from .posterior import posterior_covariance
    if moho is True:
        moho = [tuple(float(v) for v in saved_priors(p)["z"]) for p in datapaths]
    rows, site = _stack_sites([np.load(op.join(p, "c_models.npy")) for p in datapaths])
    return posterior_covariance(rows, site=site, dep_int=dep_int, moho=moho, mohovs=mohovs, engine=engine, nsites=len(datapaths))


def station_slots(targets_per_station):
    """(rows, missing): every station's targets as a row of slots, one slot per target reference in the order of first
    appearance, None where the station lacks it; missing = some station lacks a slot (SiteTargets(missing=True) then)"""
    refs = []
    for tl in targets_per_station:
        for t in tl:
            if t.ref not in refs:
                refs.append(t.ref)
    rows = []
    for tl in targets_per_station:
        by_ref = {t.ref: t for t in tl}
        if len(by_ref) != len(tl):
            raise ValueError("a station has two targets of one reference")
        rows.append([by_ref.get(r) for r in refs])
    return rows, any(t is None for row in rows for t in row)


def residuals_from_storage(datapaths, maxlag=10, quantiles=(0.025, 0.16, 0.5, 0.84, 0.975), laws=None, engine=None):
    """Whether the residuals of many sites' posterior models look like the noise they assumed
    (bayhunter_amd.datafits.posterior_residuals): datapaths[s] is site s's data directory after save_final_distribution
    (c_models.npy, c_vpvs.npy and c_noise.npy, the (corr, sigma) pairs of the station's own targets).  Targets, priors and the
    mantle rule are those of the saved <station>_config.pkl, as for datafits_from_storage.  The file does not say which noise law
    the sampler installed: laws, a dict target reference -> law name ("exp", "nocorr", "nocorr_scalederr") or the pair
    ("gauss", corr) of Target.set_noise_law, names them (they decide `law`, `acf_model` and the weights of nocorr_scalederr);
    references it leaves out count as "nocorr".  Returns one dict per site."""
    from .datafits import posterior_residuals
    from .sites import SiteTargets
    S = len(datapaths)
    per_station = [saved_targets(p) for p in datapaths]
    for tl in per_station:
        for t in tl:
            law = (laws or {}).get(t.ref, "nocorr")
            if isinstance(law, str):
                t.set_noise_law(law)
            else:
                t.set_noise_law(law[0], corr=law[1])
    slots, missing = station_slots(per_station)
    st = SiteTargets(slots, engine=engine, per_site_x="all", per_site_rf="all", missing=missing)
    mantle = [saved_priors(p).get("mantle") for p in datapaths]
    bands = [np.load(op.join(p, "c_models.npy")) for p in datapaths]
    rows, site = _stack_sites(bands)
    vpvs = np.concatenate([np.load(op.join(p, "c_vpvs.npy")).reshape(len(b)) for p, b in zip(datapaths, bands)])
    # every station's own (corr, sigma) pairs into the slot layout
    refs = [next(t for t in col if t is not None).ref for col in zip(*slots)]
    noise = np.zeros((len(rows), 2 * len(refs)))
    noise[:, 1::2] = 1.0
    start = 0
    for p, b, tl in zip(datapaths, bands, per_station):
        own = np.load(op.join(p, "c_noise.npy")).reshape(len(b), -1)
        for k, t in enumerate(tl):
            i = refs.index(t.ref)
            noise[start:start + len(b), 2 * i:2 * i + 2] = own[:, 2 * k:2 * k + 2]
        start += len(b)
    return posterior_residuals(st, rows, vpvs, noise, site=site, maxlag=maxlag, quantiles=quantiles, mantle=mantle, engine=engine,
                               nsites=S)


def datafits_from_storage(datapaths, quantiles=(0.025, 0.16, 0.5, 0.84, 0.975), dev=0.05, engine=None):
    """Best data fits and posterior predictive bands of many sites (bayhunter_amd.datafits.posterior_datafits, the numbers of the
    reference's plot_bestdatafits and more): datapaths[s] is site s's data directory.  The best fits come from the main-phase
    chain files c???_p2{models,vpvs,misfits}.npy, outlier chains (get_outliers with `dev`) left out as the reference's plot
    leaves them out; the bands from c_models.npy / c_vpvs.npy (save_final_distribution).  Targets, priors and the mantle rule
    are those of the saved <station>_config.pkl; stations whose configs differ in their targets become the slots of a
    SiteTargets(missing=True) (`station_slots`).  Returns one dict per site; the `row` of a best fit counts the rows of its own
    chain file (`chain` is the file's chain index)."""
    from .datafits import posterior_datafits, best_rows
    from .sites import SiteTargets
    S = len(datapaths)
    slots, missing = station_slots([saved_targets(p) for p in datapaths])
    st = SiteTargets(slots, engine=engine, per_site_x="all", per_site_rf="all", missing=missing)
    mantle = [saved_priors(p).get("mantle") for p in datapaths]
    # the chain files of every station: the rows of the best fits
    cm, cv, cf, cc, cs, crow = [], [], [], [], [], []
    for s, p in enumerate(datapaths):
        outliers = get_outliers(p, dev=dev)
        for f in _chainfiles(p, 2, "models"):
            ci = _chainidx(f)
            if ci in outliers:
                continue
            m = np.load(f)
            cm.append(m)
            cv.append(np.load(f.replace("models", "vpvs")).reshape(len(m)))
            cf.append(np.load(f.replace("models", "misfits")).reshape(len(m), -1)[:, -1])
            cc.append(np.full(len(m), ci, np.int32))
            cs.append(np.full(len(m), s, np.int32))
            crow.append(np.arange(len(m)))
    bands = [np.load(op.join(p, "c_models.npy")) for p in datapaths]
    rows, site = _stack_sites(bands)
    vpvs = np.concatenate([np.load(op.join(p, "c_vpvs.npy")).reshape(len(b)) for p, b in zip(datapaths, bands)])
    out = posterior_datafits(st, rows, vpvs, site=site, quantiles=quantiles, mantle=mantle, engine=engine, nsites=S)
    if cm:
        brow, bsite = _stack_sites(cm)
        bsite = np.concatenate(cs)
        crow = np.concatenate(crow)
        cv, cc, cf = np.concatenate(cv), np.concatenate(cc), np.concatenate(cf)
        # the winners first (no forward model runs for that); only they go through the targets
        win = best_rows(brow, bsite, cc, cf, S, engine=engine)
        win = np.sort(win[win >= 0])
        crow = crow[win]
        best = posterior_datafits(st, brow[win], cv[win], site=bsite[win], chain=cc[win], misfits=cf[win], quantiles=(), mantle=mantle,
                                  engine=engine, nsites=S)
        for s in range(S):
            for b in best[s]["best"]:
                b["row"] = int(crow[b["row"]])
            out[s]["best"], out[s]["thebest"] = best[s]["best"], best[s]["thebest"]
    return out
