"""Posterior data fits of many sites on the GPU (include/bh_engine_posterior_datafit.h).

`posterior_datafits` answers, for every station of a many-station run in one call, what BayHunter's
PlotFromStorage.plot_bestdatafits / plot_bestmodels answer one model at a time -- the model of least joint misfit of every
chain, turned back into layers and run through every target's forward model -- and one step more: the posterior predictive
band, i.e. count, min, max, median, mean, std and any quantiles of the synthetic data at every period and time sample over
the station's WHOLE posterior.  The rows go through bh_posterior_layers -> bh_evaluate_sites -> bh_posterior_data_fill in
forward batches of a fixed size; the synthetics become the scalar set DATA, whose per-site column passes are those of
`posterior_scalars`, and bh_posterior_scalar_quantiles selects all the ranks of a column in one read per radix pass.

`posterior_residuals` (include/bh_engine_posterior_resid.h) runs the same forward pass and keeps, instead of the
synthetics, what their residuals say about the noise every row assumed -- amplitude against sigma, lag-1 correlation against corr,
the autocorrelation function -- as the scalar set RESID; `posterior_datafits(residuals=)` forms both sets from one pass.

Exactness: the layers are the reference's Model.get_vp_vs_h and rho = vp * 0.32 + 0.77 in the dtypes numpy
computes them in; count, min, max, median and the order statistics are bit-exact functions of the synthetics; the quantiles
are numpy.quantile(..., method="linear") of them; mean and std come from exact integer sums.
"""
import ctypes as C

import numpy as np

from . import engine as E
from .posterior import _Loaded, _keys_to_values, _mean_std, _ptr, _stat_dict, median_of_middles
from .posterior import quantile_lerp, quantile_rank, set_quantiles   # noqa: F401 (the quantile formula lives with _Loaded)

DEFAULT_QUANTILES = (0.025, 0.16, 0.5, 0.84, 0.975)
DEFAULT_MAX_BYTES = 1 << 31   # of the DATA set of one group of sites
DEFAULT_BATCH = 16384         # rows of one forward batch


# ---- the pure parts: planner (the quantile formula: posterior.quantile_rank, quantile_lerp) --------------------------------

def plan_site_groups(rows, ldy, max_bytes, extra=0):
    """Sites 0..S-1 with rows[s] rows each into consecutive groups [(s0, s1), ...] whose DATA sets (ldy * rows * 8 bytes) stay
    within max_bytes; a site is never split, so a site that alone exceeds the budget is a group of its own.  extra: the columns
    of a set formed beside the DATA set (the RESID set), counted likewise; ldy may then be 0 (no DATA set)."""
    rows = [int(r) for r in rows]
    if ldy < 0 or extra < 0 or ldy + extra < 1 or max_bytes < 1 or any(r < 0 for r in rows):
        raise ValueError("ldy and max_bytes must be positive, rows non-negative")
    groups, s0, used = [], 0, 0
    for s, r in enumerate(rows):
        need = r * (ldy + extra) * 8
        if s > s0 and used + need > max_bytes:
            groups.append((s0, s))
            s0, used = s, 0
        used += need
    if rows:
        groups.append((s0, len(rows)))
    return groups


def plan_batches(nrows, batch):
    """The loaded rows 0..nrows-1 as consecutive forward batches [(r0, r1), ...] of `batch` rows (the last one shorter)."""
    if batch < 1 or nrows < 0:
        raise ValueError("batch must be positive, nrows non-negative")
    return [(r0, min(r0 + batch, nrows)) for r0 in range(0, nrows, batch)]


# ---- the handle's calls ----------------------------------------------------------------------------------------------------

def _is_tensor(a):
    try:
        import torch
        return isinstance(a, torch.Tensor)
    except ImportError:
        return False


def _per_row(a, N, what, ints=False):
    """one value per input row as (memspace, stream, pointer, stride, element bytes, the array kept alive)"""
    if _is_tensor(a):
        import torch
        a = a.reshape(N)
        if ints:
            a = a.to(torch.int32)
        elif a.dtype not in (torch.float32, torch.float64):
            a = a.to(torch.float64)
        return E.DEVICE, C.c_void_p(torch.cuda.current_stream(a.device).cuda_stream), C.c_void_p(a.data_ptr()), a.stride(0) if N else 1, \
            a.element_size(), a
    a = np.asarray(a)
    if a.size != N:
        raise ValueError("%s: one value per model row" % what)
    a = a.reshape(N)
    if ints:
        a = np.ascontiguousarray(a, np.int32)
    elif a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float64)
    a = np.ascontiguousarray(a)
    return E.HOST, None, _ptr(a), 1, a.itemsize, a


class _DataLoaded(_Loaded):
    """_Loaded with the calls of include/bh_engine_posterior_datafit.h"""

    def __init__(self, models, site, engine, nsites=None):
        _Loaded.__init__(self, models, site, engine, nsites, scalars=True)
        self.nrows = int(self.rows.sum())

    def layers(self, r0, r1, vpvs, mantle_vs, mantle_vpvs, out, stride_l):
        """vpvs: the tuple of _per_row; out: dict of device tensors nlay, h, vp, vs, rho, site"""
        mem, stream, ptr, stride, elem, _ = vpvs
        p = lambda k: C.c_void_p(out[k].data_ptr())
        self.eng._check(self._L.bh_posterior_layers(self._p, r0, r1, mem, stream, elem, stride, ptr, _ptr(mantle_vs), _ptr(mantle_vpvs),
                                                    p("nlay"), p("h"), p("vp"), p("vs"), p("rho"), stride_l, p("site")))

    def best(self, nchains, chain, misfits):
        cm, cs, cp, cst, _, ckeep = _per_row(chain, self.N, "chain", ints=True)
        mm, ms, mp, mst, mel, mkeep = _per_row(misfits, self.N, "misfits")
        if cm != mm:                                   # one memspace per call: the host one comes to the device
            import torch
            dev = (ckeep if cm == E.DEVICE else mkeep).device
            if cm == E.HOST:
                cm, cs, cp, cst, _, ckeep = _per_row(torch.from_numpy(ckeep).to(dev), self.N, "chain", ints=True)
            else:
                mm, ms, mp, mst, mel, mkeep = _per_row(torch.from_numpy(mkeep).to(dev), self.N, "misfits")
        best = np.zeros((self.S, nchains), np.int64)
        pos = np.zeros((self.S, nchains), np.int64)
        self.eng._check(self._L.bh_posterior_best(self._p, int(nchains), cm, cs, cp, cst, mel, mp, mst, _ptr(best), _ptr(pos)))
        return best, pos

    def data_fill(self, stream, r0, nb, ldy, ymod, err, ncol):
        ncol = np.ascontiguousarray(ncol, np.int32)
        failed = np.zeros(self.S, np.int64)
        self.eng._check(self._L.bh_posterior_data_fill(self._p, stream, r0, nb, ldy, C.c_void_p(ymod.data_ptr()) if ymod is not None else None,
                                                       C.c_void_p(err.data_ptr()) if err is not None else None, ncol.shape[1],
                                                       _ptr(ncol), _ptr(failed)))
        return failed

    def resid_fill(self, stream, r0, nb, ldy, ymod, err, ncol, L, yobs, g, noise):
        """bh_posterior_resid_fill (include/bh_engine_posterior_resid.h); noise: the tuple of _noise_rows; yobs, g: float64
        [S, ldy], g may be None"""
        ncol = np.ascontiguousarray(ncol, np.int32)
        failed = np.zeros(self.S, np.int64)
        mem, elem, nld, nptr, _ = noise
        self.eng._check(self._L.bh_posterior_resid_fill(self._p, stream, r0, nb, ldy, C.c_void_p(ymod.data_ptr()) if ymod is not None else None,
                                                        C.c_void_p(err.data_ptr()) if err is not None else None, ncol.shape[1],
                                                        _ptr(ncol), int(L), _ptr(yobs), _ptr(g), mem, elem, nld, nptr, _ptr(failed)))
        return failed


def _noise_rows(noise, N, nt):
    """the noise table, one row [>= 2 nt] of (corr, sigma) pairs per model row in the slot layout of samples(), as (memspace,
    element bytes, leading dimension, pointer, the array kept alive); float32 / float64, numpy array or device tensor"""
    if noise is None:
        raise ValueError("noise is needed: one row of (corr, sigma) pairs per model row")
    if _is_tensor(noise):
        import torch
        a = noise.reshape(N, -1) if N else noise.reshape(0, 2 * nt)
        if a.dtype not in (torch.float32, torch.float64):
            a = a.to(torch.float64)
        if a.shape[1] < 2 * nt:
            raise ValueError("noise: %d values per row, the targets need %d" % (a.shape[1], 2 * nt))
        if N and (a.stride(1) != 1 or a.stride(0) < a.shape[1]):
            a = a.contiguous()
        return E.DEVICE, a.element_size(), (a.stride(0) if N > 1 else a.shape[1]), C.c_void_p(a.data_ptr()), a
    a = np.asarray(noise)
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float64)
    a = np.ascontiguousarray(a.reshape(N, -1) if N else a.reshape(0, 2 * nt))
    if a.shape[1] < 2 * nt:
        raise ValueError("noise: %d values per row, the targets need %d" % (a.shape[1], 2 * nt))
    return E.HOST, a.itemsize, a.shape[1], _ptr(a), a


class _Clock(object):
    """seconds per phase into a dict (tools/gpu_posterior_datafits_perf.py), the device drained at every lap; nothing without one"""

    def __init__(self, into, dev):
        import time
        self.into, self.dev, self.now = into, dev, time.perf_counter
        self.t = self.now()

    def lap(self, name):
        if self.into is None:
            return
        import torch
        torch.cuda.synchronize(self.dev)
        t = self.now()
        self.into[name] = self.into.get(name, 0.0) + (t - self.t)
        self.t = t


class _Forward(object):
    """The device buffers of one forward batch and the loop rows -> layers -> bh_evaluate_sites -> DATA set."""

    def __init__(self, eng, dev, B, ML, nt, ldy):
        import torch
        self.eng, self.dev, self.B, self.ML, self.nt, self.ldy = eng, dev, B, ML, nt, ldy
        self.stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self.buf = dict(nlay=z(B, torch.int32), site=z(B, torch.int32), err=z(B, torch.int32), logL=z(B, torch.float64),
                        misf=z((B, nt + 1), torch.float64), ymod=z((B, ldy), torch.float64),
                        noise=torch.tensor([0.0, 1.0] * nt, dtype=torch.float64, device=dev).repeat(B, 1).contiguous())
        for k in ("h", "vp", "vs", "rho"):
            self.buf[k] = z((ML, B), torch.float64)
        torch.cuda.synchronize(dev)

    def fill(self, ld, vpvs, mantle_vs, mantle_vpvs, s0, ncol, clock=None, data=True, resid=None):
        """Form the DATA set of the loaded rows (data), the RESID set (resid: a dict of L, yobs, g and noise, the tuple of
        _noise_rows, for the loaded sites) or both from one forward pass; site indices of the load + s0 are the targets' sites.
        Returns failed[S]."""
        buf, B, ML = self.buf, self.B, self.ML
        ptr = lambda k: C.c_void_p(buf[k].data_ptr())
        failed = np.zeros(ld.S, np.int64)
        rfill = lambda r0, nb, ymod, err: ld.resid_fill(self.stream, r0, nb, self.ldy, ymod, err, ncol, resid["L"], resid["yobs"],
                                                        resid["g"], resid["noise"])
        if ld.nrows == 0:
            if data:
                failed = ld.data_fill(self.stream, 0, 0, self.ldy, None, None, ncol)
            if resid is not None:
                failed = rfill(0, 0, None, None)
        for r0, r1 in plan_batches(ld.nrows, B):
            nb = r1 - r0
            ld.layers(r0, r1, vpvs, mantle_vs, mantle_vpvs, buf, B)
            if s0:
                buf["site"][:nb] += s0
            if clock is not None:
                clock.lap("layers")
            self.eng.evaluate_sites_dev(nb, ML, ptr("nlay"), ptr("h"), ptr("vp"), ptr("vs"), ptr("rho"), B, 1, ptr("site"), ptr("noise"),
                                        ptr("logL"), ptr("misf"), ptr("err"), ymod=ptr("ymod"), stream=self.stream)
            if clock is not None:
                clock.lap("forward")
            if data:
                failed = ld.data_fill(self.stream, r0, nb, self.ldy, buf["ymod"], buf["err"], ncol)
                if clock is not None:
                    clock.lap("fill")
            if resid is not None:
                failed = rfill(r0, nb, buf["ymod"], buf["err"])
                if clock is not None:
                    clock.lap("residuals")
        return failed


# ---- the public call ---------------------------------------------------------------------------------------------------------

def best_rows(models, site, chain, misfits, nsites, engine=None):
    """int64 [nsites, nchains]: the row of the first least misfit of every (site, chain) (bh_posterior_best alone: nothing goes
    through a forward model), -1 where the pair has no row; nchains = the largest chain id + 1"""
    N = models.shape[0]
    nchains = max(int(_host(chain).reshape(N).max()) + 1, 1) if N else 1
    ld = _DataLoaded(models, site, engine, nsites)
    try:
        return ld.best(nchains, chain, misfits)[0]
    finally:
        ld.close()


def _as_sites(targets, engine):
    from .sites import SiteTargets
    if isinstance(targets, SiteTargets):
        if engine is not None and targets._engine is None:
            targets._engine = engine
        return targets, True
    return SiteTargets([targets], engine=engine), False


def _mantle_arrays(mantle, S):
    """None, one (vs, vpvs) pair or one pair / None per site -> (mantle_vs[S], mantle_vpvs[S]) or (None, None)"""
    if mantle is None:
        return None, None
    m = list(mantle)
    if len(m) == 2 and not isinstance(m[0], (tuple, list, np.ndarray, type(None))):
        m = [m] * S
    if len(m) != S:
        raise ValueError("mantle: one (vs, vpvs) pair or one per site")
    mv, mk = np.full(S, -1.0), np.zeros(S)
    for s, pair in enumerate(m):
        if pair is not None:
            mv[s], mk[s] = float(pair[0]), float(pair[1])
    return mv, mk


def _take(a, idx):
    """rows idx (numpy int64) of a numpy array or device tensor"""
    if _is_tensor(a):
        import torch
        return a[torch.from_numpy(idx).to(a.device)]
    return np.asarray(a)[idx]


def _host(a):
    return a.detach().cpu().numpy() if _is_tensor(a) else np.asarray(a)


def posterior_datafits(targets, models, vpvs, site=None, chain=None, misfits=None, noise=None, quantiles=DEFAULT_QUANTILES,
                       mantle=None, engine=None, nsites=None, max_bytes=DEFAULT_MAX_BYTES, residuals=None):
    """Best fits per chain and the posterior predictive band of every datum, for every site: a list of dicts (one dict where
    `targets` is a JointTarget).

    targets: a JointTarget (one site) or a SiteTargets with any of its flags; the call registers it on its engine and evaluates
    through bh_evaluate_sites on device pointers.  models: rows [vs_1..vs_n, z_1..z_n, NaN...] (float32 / float64; numpy array or
    device tensor) and vpvs one value per row, as for posterior_moho; site: every row's site index (device rows with an index
    out of range, e.g. -1, are left out).  mantle: None, one (mantle_vs, mantle_vpvs) pair or one pair / None per site: the
    reference's mantle rule for vp.  noise only feeds the likelihood, which the call discards: every evaluation runs with corr 0
    and sigma 1, and a given `noise` is not read.

    Every dict holds rows (the site's rows), failed (the rows whose forward model failed: they are masked in every column) and,
    per target reference ("rdispph", "prf", ...; under missing=True the site's own targets): x, obs, and per datum count, nan (the
    masked rows), min, max, median, mean, std and quantiles [R, n] (numpy.quantile, method "linear", of the site's synthetics; NaN where count is
    0).  With chain (int, 0 <= chain) and misfits (the joint misfit) per row: best = a list, per chain that has rows, of dicts
    chain, row (index into `models`; the first least misfit, numpy.argmin), misfit, model (the row), vpvs and data (target
    reference -> synthetics; NaN where that model's forward run failed), and thebest = the first of them with the least misfit.

    The DATA set takes ldy * rows * 8 bytes of device memory: where that exceeds max_bytes the sites are split into groups
    (`plan_site_groups`; sites are independent) that are loaded one after the other; `batch` rows go through the forward
    kernels at a time (`plan_batches`; DEFAULT_BATCH).

    What leaves the device when the rows are device tensors: `site` comes to the host once (N int32: the rows per site, which
    the planner of the groups needs), and so do `chain` and `misfits` where given (the number of chains, the misfits of the result
    dicts), and the rows of the best fits; models, vpvs and all synthetics stay where they are.

    The engine's search and arithmetic settings are the caller's.  With the engine's defaults (the short refinement, the fast
    arithmetic) the dispersion columns carry the documented 2e-6 relative deviation of the short refinement from the
    reference's root search; select set_swd_search("reference") and set_swd_arith("exact") for the reference's bits.

    residuals: None, or a dict {"noise": ..., "maxlag": 10} (and "quantiles", default: those of this call) as posterior_residuals
    takes them: every target's dict gains the key `residuals`, the dict posterior_residuals returns for it, formed from the same
    forward pass.  With None nothing of it runs."""
    return _datafits(targets, models, vpvs, site, chain, misfits, quantiles, mantle, engine, nsites, max_bytes, residuals=residuals)


RESID_NAMES = ("bias", "rms", "sigma_ratio", "corr", "corr_excess")   # the columns of a slot before its autocorrelation function


def posterior_residuals(targets, models, vpvs, noise, site=None, maxlag=10, quantiles=DEFAULT_QUANTILES, mantle=None, engine=None,
                        nsites=None, max_bytes=DEFAULT_MAX_BYTES):
    """Is the assumed noise the noise?  For every site the posterior of what the residuals of its models say about the noise law
    the rows themselves carry: a list of dicts (one dict where `targets` is a JointTarget).  targets, models, vpvs, site, mantle,
    engine, nsites and max_bytes as for posterior_datafits, whose forward pass this is (corr 0 and sigma 1; the likelihood is
    discarded).  noise: one row [2 nt] per model row (float32 / float64; numpy array or device tensor), (corr, sigma) of slot t at
    2t, 2t + 1 -- the slot layout of samples() -- read, unlike posterior_datafits', by bh_posterior_resid_fill
    (include/bh_engine_posterior_resid.h), which forms per (row, slot) from e = ymod - yobs:
      bias = mean e;  rms = sqrt(mean e^2), the reference's misfit;  sigma_ratio = sqrt(mean u^2) / sigma, about 1 where the noise
      model is right;  corr, the row's own;  corr_excess = acf_1 - corr;  acf_l = sum u_i u_{i+l} / sum u_i^2 at the lags
      l = 1 .. maxlag (at most 32), with u = e * g and g = 1 / sqrt(yerr / min yerr) where the slot's law is nocorr_scalederr,
      else 1.
    Every dict holds rows, failed (the rows whose forward model failed: NaN in every column) and per target reference ("rdispph",
    "prf", ...; under missing=True the site's own targets) a dict of n, law (the one installed at the site), lags = 1 .. maxlag; for
    each of bias, rms, sigma_ratio, corr, corr_excess a dict of count, nan, min, max, median, mean, std, quantiles [R]; acf: the same
    keys with arrays [maxlag] and quantiles [R, maxlag]; acf_model [maxlag]: the curve the law implies at the posterior median r of
    corr -- r^l (exp), r^(l^2) (gauss), 0 (nocorr, nocorr_scalederr); and acf_white95 = 1.96 / sqrt(n), the band a white
    residual's acf stays in 95 % of the time.  Statistics are those of posterior_scalars on the same columns, bit for bit."""
    return _datafits(targets, models, vpvs, site, None, None, quantiles, mantle, engine, nsites, max_bytes,
                     residuals=dict(noise=noise, maxlag=maxlag), data=False)


def _resid_tables(st):
    """(yobs [S, ldy], g [S, ldy] or None, the law names [S][nt]): the observed data in the DATA set's column blocks, and
    1 / sqrt(yerr / min yerr) where the (site, slot)'s installed law is nocorr_scalederr (the reference scales the variance by
    that factor), 1 elsewhere; None where no slot is under that law"""
    n = st._counts()
    off = np.concatenate(([0], np.cumsum(n.max(axis=0)))).astype(int)
    yobs, g, laws = np.zeros((st.nsites, off[-1])), None, []
    for s, row in enumerate(st._slot_rows()):
        laws.append([None if t is None else t.law() for t in row])
        for i, t in enumerate(row):
            if t is None:
                continue
            c = slice(off[i], off[i] + n[s, i])
            yobs[s, c] = np.asarray(t.obsdata.y, dtype=float).ravel()
            if laws[s][i] == "nocorr_scalederr":
                if g is None:
                    g = np.ones_like(yobs)
                ye = np.asarray(t.obsdata.yerr, dtype=float).ravel()
                g[s, c] = 1.0 / np.sqrt(ye / ye.min())
    return yobs, g, laws


def acf_model(law, r, L):
    """the autocorrelation a noise law implies at the lags 1 .. L for the correlation r: r^l (exp), r^(l^2) (gauss), 0 (the
    uncorrelated laws)"""
    lags = np.arange(1, L + 1, dtype=np.float64)
    if law == "exp":
        return np.float64(r) ** lags
    if law == "gauss":
        return np.float64(r) ** (lags * lags)
    return np.zeros(L)


def _resid_dict(stt, qv, g, q0, L, n, law):
    """one (site, slot)'s result from the statistics and quantiles [S, Q, R] of the RESID set; q0: the slot's first column"""
    def col(q):
        d = dict(count=int(stt["count"][g, q]), nan=int(stt["nan"][g, q]))
        d.update(_stat_dict(stt, g, q))
        d["quantiles"] = qv[g, q].copy()
        return d
    out = dict(n=int(n), law=law, lags=np.arange(1, L + 1))
    for k, name in enumerate(RESID_NAMES):
        out[name] = col(q0 + k)
    lags = [col(q0 + E.RESID_FIXED + l) for l in range(L)]
    out["acf"] = {k: np.array([d[k] for d in lags]) for k in ("count", "nan", "min", "max", "median", "mean", "std")}
    out["acf"]["quantiles"] = np.ascontiguousarray(np.array([d["quantiles"] for d in lags]).reshape(L, -1).T)
    out["acf_model"] = acf_model(law, out["corr"]["median"], L)
    out["acf_white95"] = 1.96 / np.sqrt(n) if n else np.nan
    return out


def _datafits(targets, models, vpvs, site=None, chain=None, misfits=None, quantiles=DEFAULT_QUANTILES, mantle=None, engine=None,
              nsites=None, max_bytes=DEFAULT_MAX_BYTES, batch=DEFAULT_BATCH, timing=None, residuals=None, data=True):
    """posterior_datafits with the rows of a forward batch and a dict for the seconds per phase (tests, tools); data=False: the
    RESID set alone (posterior_residuals)"""
    import torch
    st, many = _as_sites(targets, engine)
    eng = st.engine
    st._register()
    S, nt, ldy = st.nsites, st.ntargets, eng.ldy
    if ldy > E.DATAFIT_MAXCOLS:
        raise ValueError("%d data columns: at most %d (BH_DATAFIT_MAXCOLS)" % (ldy, E.DATAFIT_MAXCOLS))
    RL = RQ = 0
    if residuals is not None:
        unknown = [k for k in residuals if k not in ("noise", "maxlag", "quantiles")]
        if unknown:
            raise ValueError("residuals: no key %r (noise, maxlag, quantiles)" % (unknown[0],))
        RL = int(residuals.get("maxlag", 10))
        if not 1 <= RL <= E.RESID_MAXLAG:
            raise ValueError("maxlag: 1..%d (BH_RESID_MAXLAG)" % E.RESID_MAXLAG)
        RQ = nt * (E.RESID_FIXED + RL)
        if RQ > E.DATAFIT_MAXCOLS:
            raise ValueError("%d residual columns: at most %d (BH_DATAFIT_MAXCOLS)" % (RQ, E.DATAFIT_MAXCOLS))
        rqs = tuple(float(q) for q in residuals.get("quantiles", quantiles))
        rnoise = residuals.get("noise")
        if rnoise is None:
            raise ValueError("residuals: noise is needed, one row of (corr, sigma) pairs per model row")
        if not _is_tensor(rnoise):
            rnoise = np.asarray(rnoise)
        if rnoise.shape[0] != models.shape[0]:
            raise ValueError("noise: one row per model row")
        ryobs, rg, rlaws = _resid_tables(st)
    if nsites is not None and int(nsites) != S:
        raise ValueError("nsites=%d, the targets have %d sites" % (nsites, S))
    ncol = st._counts()
    cap = ncol.max(axis=0)
    off = np.concatenate(([0], np.cumsum(cap))).astype(int)
    if off[-1] != ldy:
        raise ValueError("the targets' columns do not add up to the engine's ldy")
    if not _is_tensor(vpvs):
        vpvs = np.asarray(vpvs)
    N = models.shape[0]
    qs = tuple(float(q) for q in quantiles)
    mv, mk = _mantle_arrays(mantle, S)
    if (chain is None) != (misfits is None):
        raise ValueError("chain and misfits go together")
    # rows per site, for the groups
    if site is None:
        if S != 1:
            raise ValueError("site is needed with more than one site")
        per_site = np.array([N])
        hsite = None
    else:
        hsite = _host(site).astype(np.int64).reshape(N)
        ok = (hsite >= 0) & (hsite < S)
        per_site = np.bincount(hsite[ok], minlength=S)
    groups = plan_site_groups(per_site, ldy if data else 0, int(max_bytes), extra=RQ)
    nchains = 0
    if chain is not None:
        hchain, hmis = _host(chain).reshape(N), _host(misfits).reshape(N)
        nchains = max(int(hchain.max()) + 1, 1) if N else 1
    dev = models.device if _is_tensor(models) else torch.device("cuda", eng.device)
    out = [None] * S
    clock = _Clock(timing, dev)
    with torch.cuda.device(dev):
        fw = _Forward(eng, dev, int(batch), models.shape[1] // 2, nt, ldy)
        for s0, s1 in groups:
            whole = (s0, s1) == (0, S)
            if whole:
                idx, gm, gv, gs, gc, gf = None, models, vpvs, site, chain, misfits
                gn = rnoise if residuals is not None else None
            else:
                idx = np.flatnonzero((hsite >= s0) & (hsite < s1))
                gm, gv = _take(models, idx), _take(vpvs, idx)
                gs = (hsite[idx] - s0).astype(np.int32)
                if _is_tensor(models):
                    gs = torch.from_numpy(gs).to(dev)
                gc = None if chain is None else _take(chain, idx)
                gf = None if misfits is None else _take(misfits, idx)
                gn = _take(rnoise, idx) if residuals is not None else None
            clock.lap("host")
            ld = _DataLoaded(gm, gs, eng, s1 - s0)
            clock.lap("load")
            try:
                G = s1 - s0
                # vpvs on the device once: the layer calls read it batch after batch
                gvt = gv if _is_tensor(gv) else torch.from_numpy(np.ascontiguousarray(np.asarray(gv).reshape(ld.N))).to(dev)
                vt = _per_row(gvt, ld.N, "vpvs")
                gmv, gmk = (None, None) if mv is None else (np.ascontiguousarray(mv[s0:s1]), np.ascontiguousarray(mk[s0:s1]))
                best = pos = None
                if chain is not None:
                    best, pos = ld.best(nchains, gc, gf)
                    clock.lap("best")
                resid = None
                if residuals is not None:
                    resid = dict(L=RL, yobs=np.ascontiguousarray(ryobs[s0:s1]), g=None if rg is None else np.ascontiguousarray(rg[s0:s1]),
                                 noise=_noise_rows(gn, ld.N, nt))
                failed = fw.fill(ld, vt, gmv, gmk, s0, ncol[s0:s1], clock, data=data, resid=resid)
                bdata = None
                if data:
                    stt = ld.scalar_stats(E.SCALARS_DATA)
                    clock.lap("statistics")
                    qv = set_quantiles(ld, E.SCALARS_DATA, stt["count"], qs) if qs else np.zeros((G, ldy, 0))
                    clock.lap("quantiles")
                    if best is not None and (pos >= 0).any():
                        bdata = ld.gather(E.SCALARS_DATA, pos[pos >= 0], ldy)
                if residuals is not None:
                    rstt = ld.scalar_stats(E.SCALARS_RESID)
                    clock.lap("residual statistics")
                    rqv = set_quantiles(ld, E.SCALARS_RESID, rstt["count"], rqs) if rqs else np.zeros((G, RQ, 0))
                    clock.lap("residual quantiles")
            finally:
                ld.close()
            clock.lap("host")
            taken = 0
            for g in range(G):
                s = s0 + g
                n_rows = int(ld.rows[g])
                r = dict(rows=n_rows, failed=int(failed[g]))
                slots = st._slot_rows()[s]
                for t, tgt in enumerate(slots):
                    if tgt is None:
                        continue
                    rd = None
                    if residuals is not None:
                        rd = _resid_dict(rstt, rqv, g, t * (E.RESID_FIXED + RL), RL, int(ncol[s, t]), rlaws[s][t])
                    if not data:
                        r[tgt.ref] = rd
                        continue
                    c0, c1 = off[t], off[t] + int(ncol[s, t])
                    cnt = stt["count"][g, c0:c1]
                    d = dict(x=np.asarray(tgt.obsdata.x, dtype=float), obs=np.asarray(tgt.obsdata.y, dtype=float), count=cnt.copy(),
                             nan=stt["nan"][g, c0:c1].copy())
                    for k in ("min", "max", "median", "mean", "std"):
                        d[k] = np.full(c1 - c0, np.nan)
                    for j, q in enumerate(range(c0, c1)):
                        n = int(cnt[j])
                        if not n:
                            continue
                        d["min"][j], d["max"][j] = stt["min"][g, q], stt["max"][g, q]
                        d["median"][j] = median_of_middles(stt["med"][g, q, 0], stt["med"][g, q, 1], n)
                        d["mean"][j], d["std"][j] = _mean_std(n, stt["sums"][g, q], stt["scale"][g, q], stt["x0"][g, q])
                    d["quantiles"] = np.ascontiguousarray(qv[g, c0:c1].T)
                    if rd is not None:
                        d["residuals"] = rd
                    r[tgt.ref] = d
                if best is not None:
                    r["best"] = []
                    for c in range(nchains):
                        if best[g, c] < 0:
                            continue
                        i = int(best[g, c]) if idx is None else int(idx[best[g, c]])
                        row = bdata[taken]
                        taken += 1
                        r["best"].append(dict(chain=c, row=i, misfit=hmis[i], model=_host(models[i]), vpvs=_host(vpvs.reshape(N)[i])[()],
                                              data={tgt.ref: row[off[t]:off[t] + int(ncol[s, t])].copy()
                                                    for t, tgt in enumerate(slots) if tgt is not None}))
                    mis = [b["misfit"] for b in r["best"]]
                    r["thebest"] = r["best"][int(np.argmin(mis))] if mis else None
                out[s] = r
            clock.lap("host")
    return out if many else out[0]
