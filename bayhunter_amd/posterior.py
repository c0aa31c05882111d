"""Posterior velocity-depth summaries of many sites on the GPU (include/bh_engine_posterior.h).

`posterior_models` returns per site what BayHunter's ModelMatrix.get_singlemodels returns (mean, median, minmax,
stdminmax, mode, minmisfit) plus `count`, `mode_valid` and `invalid_rows`; `posterior_hist2d` returns the numbers of the
2-D posterior plot (the vs-depth histogram and the histogram of interface depths).  Rows are the reference's
[vs_1..vs_n, z_1..z_n, NaN...], float32 or float64, numpy arrays or device torch tensors, with a site index each.

Exactness ("Posterior summaries"): min, max, median, counts, histograms and mode are the reference's bits.
The mean and std come from exact integer sums formed on the device (every interpolated vs is an integer multiple of the
column's lowest set bit); they are rounded here from Python integers, within one rounding of the exact values.

`posterior_moho` and `posterior_scalars` (include/bh_engine_posterior_scalars.h) return per site the numbers of the
reference's plot_moho_crustvel_tradeoff and plot_posterior_likes / _misfits / _nlayers / _vpvs / _noise / _others: Moho
depth, crustal vs and any scalar column attached to the rows, with the same exactness.

`posterior_covariance` (include/bh_engine_posterior_cov.h) returns per site the mean vector and the covariance and correlation
matrices of the vs at the depths of dep_int, and of scalar columns beside them: how the depths of a profile vary together.

`posterior_features` (include/bh_engine_posterior_features.h) returns per site the posteriors of structural features of the
layered models themselves -- layer averages and travel times of a depth window, its slowest and fastest layer, its strongest
velocity drop and jump, the first interface above a velocity, the number of interfaces -- each with the statistics of
posterior_scalars and, where a feature may be absent, the posterior probability that it is there.

`posterior_classes` (include/bh_engine_posterior_classes.h) splits every site's rows into classes by a rule over those scalar
columns -- a Moho at 30-36 km or at 36-45 km, a low-velocity zone that is there or not -- and `classes=` of the functions above
summarises every class of every site on its own: the conditional posteriors of a bimodal station.
"""
import ctypes as C
import math

import numpy as np

from . import engine as E

VS_INTERVAL = 0.025  # km/s: the mode's vs bin width (get_singlemodels) and the 2-D plot's
MAX_COUNTS = 1 << 27  # BH_POSTERIOR_MAXCOUNTS: histogram cells of one call


def default_dep_int():
    return np.linspace(0, 100, 201)


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _keys_to_values(k, keys32):
    """The inverse of the ordered-key map of include/bh_engine_posterior.h."""
    k = np.asarray(k, dtype=np.uint64)
    if keys32:
        u = k.astype(np.uint32)
        neg = (u >> np.uint32(31)) == 0
        u = np.where(neg, ~u, u & np.uint32(0x7fffffff)).astype(np.uint32)
        return u.view(np.float32).astype(np.float64)
    neg = (k >> np.uint64(63)) == 0
    u = np.where(neg, ~k, k & np.uint64(0x7fffffffffffffff)).astype(np.uint64)
    return u.view(np.float64)


def quantile_rank(n, p):
    """(k, g) of numpy.quantile(..., method="linear") over n values: the virtual index (n - 1) * p in float64, its floor and
    the remainder; the result interpolates the order statistics k and k + 1 (k + 1 = k at the last rank)."""
    if not 0.0 <= p <= 1.0:
        raise ValueError("quantiles must be in [0, 1]")
    if n < 1:
        return 0, 0.0
    vi = np.float64(n - 1) * np.float64(p)
    k = math.floor(vi)
    if k >= n - 1:
        return n - 1, 0.0
    return int(k), float(vi - np.float64(k))


def quantile_lerp(a, b, g):
    """numpy's interpolation between the order statistics a <= b at remainder g: a + (b - a) * g, and b - (b - a) * (1 - g)
    where g >= 0.5 (float64)."""
    a, b, g = np.float64(a), np.float64(b), np.float64(g)
    d = b - a
    return b - d * (np.float64(1) - g) if g >= 0.5 else a + d * g


def check_quantiles(quantiles):
    """None, or the requested quantiles as a float64 array in the order given (duplicates allowed): a sequence of numbers in
    [0, 1]; anything else is a ValueError.  Touches no engine."""
    if quantiles is None:
        return None
    if isinstance(quantiles, (str, bytes)) or np.ndim(quantiles) != 1:
        raise ValueError("quantiles must be a sequence of numbers in [0, 1]")
    qs = []
    for q in quantiles:
        if isinstance(q, (bool, np.bool_)) or not isinstance(q, (int, float, np.integer, np.floating)):
            raise ValueError("quantiles must be numbers in [0, 1], not %r" % (q,))
        q = float(q)
        if not 0.0 <= q <= 1.0:   # (a NaN fails both)
            raise ValueError("quantiles must be in [0, 1], not %r" % (q,))
        qs.append(q)
    return np.array(qs, np.float64)


def _lerp_keys(lo, up, keys32, g, have):
    """numpy's linear interpolation at remainders g between the order statistics of the keys lo and up; NaN where not `have`"""
    a = _keys_to_values(lo.reshape(-1), keys32).reshape(lo.shape)
    b = _keys_to_values(up.reshape(-1), keys32).reshape(up.shape)
    d = b - a
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.where(g >= 0.5, b - d * (1.0 - g), a + d * g)
    return np.where(have, v, np.nan)


def set_quantiles(ld, which, count, quantiles):
    """numpy.quantile(column values, quantiles, method="linear") of every (site, column) of a set whose scalar_stats gave
    `count` [S, Q]: float64 [S, Q, R], NaN where the count is 0.  More than 8 quantiles go in several calls."""
    S, Q = count.shape
    qs = [float(q) for q in quantiles]
    out = np.full((S, Q, len(qs)), np.nan)
    for i0 in range(0, len(qs), E.QUANTILES_MAXRANKS):
        part = qs[i0:i0 + E.QUANTILES_MAXRANKS]
        rank = np.zeros((S, Q, len(part)), np.uint32)
        g = np.zeros((S, Q, len(part)))
        memo = {}
        for s in range(S):
            for q in range(Q):
                n = int(count[s, q])
                if n not in memo:
                    memo[n] = [quantile_rank(n, p) for p in part]
                for r, (k, gg) in enumerate(memo[n]):
                    rank[s, q, r], g[s, q, r] = k, gg
        lo, up = ld.quantile_keys(which, rank)
        out[:, :, i0:i0 + len(part)] = _lerp_keys(lo, up, False, g, count[:, :, None] > 0)
    return out


def column_quantiles(ld, dep, quantiles):
    """numpy.quantile(column, quantiles, method="linear") of every (site, depth) column of the interpolated vs of the loaded
    rows: float64 [S, R, D], NaN for a site without rows.  More than 8 quantiles go in several calls."""
    S, D = ld.S, len(dep)
    qs = [float(q) for q in quantiles]
    out = np.full((S, len(qs), D), np.nan)
    for i0 in range(0, len(qs), E.QUANTILES_MAXRANKS):
        part = qs[i0:i0 + E.QUANTILES_MAXRANKS]
        rank = np.zeros((S, len(part)), np.uint32)
        g = np.zeros((S, len(part)))
        for s in range(S):
            for r, p in enumerate(part):
                rank[s, r], g[s, r] = quantile_rank(int(ld.rows[s]), p)
        lo, up, k32 = ld.column_quantile_keys(dep, rank)
        v = _lerp_keys(lo, up, k32, g[:, None, :], (ld.rows > 0)[:, None, None])   # [S, D, R]
        out[:, i0:i0 + len(part), :] = v.transpose(0, 2, 1)
    return out


def depth_bins(samples, edges):
    """numpy.histogram2d's depth bin of every sample (searchsorted 'right', the last edge into the last bin); -1 outside."""
    samples, edges = np.asarray(samples, np.float64), np.asarray(edges, np.float64)
    idx = np.searchsorted(edges, samples, side="right")
    idx[samples == edges[-1]] -= 1
    return np.where((idx >= 1) & (idx <= edges.size - 1), idx - 1, -1).astype(np.int32)


def vs_round(v):
    """Down to the 0.025 km/s grid, as the reference's Plotting.vs_round rounds."""
    fl = np.floor(v)
    return fl + np.round(40 * (v - fl)) / 40


def hist2d_edges(vmin, vmax, dep_int=None):
    """The 2-D plot's default binning (_plot_bestmodels_hist): (depth sampling, depth edges) from dep_int, and for a
    site's vs range [vmin, vmax] (over the vs sampled at that depth sampling) the vs edges -- 0.025 km/s steps from two
    steps below vs_round(vmin) to below vs_round(vmax) + 3 steps."""
    if dep_int is None:
        samples, depbins = np.linspace(0, 100, 201), np.linspace(0, 100, 101)
    else:
        dep_int = np.asarray(dep_int, np.float64)
        step = dep_int[1] - dep_int[0]
        samples = np.arange(dep_int[0], dep_int[-1] + step / 2., step / 2.)
        depbins = np.arange(0, int(np.ceil(dep_int.max())) + 2 * step, step)
    if vmin is None:
        return samples, depbins, None
    lo = vs_round(vmin) - 2 * VS_INTERVAL
    hi = vs_round(vmax) + 3 * VS_INTERVAL
    return samples, depbins, np.arange(lo, hi, VS_INTERVAL)


def stepmodel(row):
    """The step model of one row (Model.get_stepmodel: vs_step, dep_step), in the row's dtype where the reference keeps it."""
    row = np.asarray(row)
    vals = row[~np.isnan(row)]
    n = vals.size // 2
    vs, z = vals[:n], vals[n:]
    zd = (z[:-1] + z[1:]) / row.dtype.type(2)
    h = np.zeros(n)
    h[:n - 1] = np.diff(np.concatenate((np.zeros(1), zd.astype(np.float64))))
    dep = np.cumsum(h)
    dep_step = np.concatenate((np.zeros(1), np.repeat(dep, 2)[:-1]))
    dep_step[-1] = max(150.0, dep_step[-1] * 2.5)
    return np.repeat(vs, 2), dep_step


class _Loaded(object):
    """Rows loaded into a bh_posterior handle (one per call of the public functions)."""

    def __init__(self, models, site, engine, nsites=None, scalars=False):
        """scalars: the load keeps what the scalar sets need (bh_posterior_keep_rows)"""
        self.eng = engine if engine is not None else E.default_engine(0)
        L = self.eng._L
        self._L = L
        h = C.c_void_p()
        self.eng._check(L.bh_posterior_create(self.eng._h, C.byref(h)))
        self._p = h
        self._keep = []
        if scalars:
            self.eng._check(L.bh_posterior_keep_rows(h, 1))
        try:
            import torch
            is_t = isinstance(models, torch.Tensor)
        except ImportError:
            is_t = False
        if is_t:
            if models.dim() != 2 or models.dtype not in (torch.float32, torch.float64) or not models.is_cuda:
                raise ValueError("models must be a 2-D float32/float64 device tensor")
            if models.stride(1) != 1:
                models = models.contiguous()
            N, W = models.shape
            ld = models.stride(0)
            elem = models.element_size()
            if site is not None:
                site = torch.as_tensor(site, device=models.device).to(torch.int32).contiguous()
                if nsites is None:
                    nsites = int(site.max().item()) + 1 if site.numel() else 1
            self._keep += [models, site]
            mptr = C.c_void_p(models.data_ptr())
            sptr = C.c_void_p(site.data_ptr()) if site is not None else None
            mem, stream = E.DEVICE, C.c_void_p(torch.cuda.current_stream(models.device).cuda_stream)
            self.dtype = np.float32 if elem == 4 else np.float64
        else:
            models = np.asarray(models)
            if models.ndim != 2 or models.dtype not in (np.float32, np.float64):
                raise ValueError("models must be a 2-D float32 or float64 array")
            models = np.ascontiguousarray(models)
            N, W = models.shape
            ld, elem = W, models.itemsize
            if site is not None:
                site = np.ascontiguousarray(site, dtype=np.int32)
                if site.shape != (N,):
                    raise ValueError("site must have one index per row")
                if nsites is None:
                    nsites = int(site.max()) + 1 if N else 1
            self._keep += [models, site]
            mptr, sptr = _ptr(models), _ptr(site)
            mem, stream = E.HOST, None
            self.dtype = models.dtype.type
        if W % 2:
            raise ValueError("rows are 2*ML values wide")
        self.S = int(nsites) if nsites is not None else 1
        self.ML = W // 2
        self.rows = np.zeros(self.S, np.int64)
        self.invalid = np.zeros(self.S, np.int64)
        dropped = np.zeros(1, np.int64)
        self.eng._check(L.bh_posterior_load(h, mem, stream, elem, N, self.ML, ld, mptr, sptr, self.S,
                                            _ptr(self.rows), _ptr(self.invalid), _ptr(dropped)))
        self.dropped = int(dropped[0])
        self.N = N
        self._keep = None

    def close(self):
        if self._p:
            self._L.bh_posterior_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def columns(self, dep, median=True):
        dep = np.ascontiguousarray(dep, np.float64)
        D, S = dep.size, self.S
        out = dict(kmin=np.zeros((S, D), np.uint64), kmax=np.zeros((S, D), np.uint64), scale=np.zeros((S, D), np.int32),
                   x0=np.zeros((S, D), np.int64), exact=np.zeros((S, D), np.int32), sums=np.zeros((S, D, 6), np.uint64),
                   median=np.zeros((S, D, 2), np.uint64) if median else None)
        k32 = np.zeros(1, np.int32)
        self.eng._check(self._L.bh_posterior_columns(self._p, D, _ptr(dep), _ptr(out["kmin"]), _ptr(out["kmax"]),
                                                     _ptr(out["scale"]), _ptr(out["x0"]), _ptr(out["exact"]),
                                                     _ptr(out["sums"]), _ptr(out["median"]), _ptr(k32)))
        out["min"] = _keys_to_values(out["kmin"], False).reshape(S, D)
        out["max"] = _keys_to_values(out["kmax"], False).reshape(S, D)
        out["keys32"] = bool(k32[0])
        return out

    def column_quantile_keys(self, dep, rank):
        """rank uint32 [S, R] -> (lower, upper, keys32): the keys [S, D, R] of every column's order statistics rank and rank + 1
        (include/bh_engine_posterior_quantiles.h)"""
        dep = np.ascontiguousarray(dep, np.float64)
        rank = np.ascontiguousarray(rank, np.uint32)
        shape = (self.S, dep.size, rank.shape[1])
        lo, up = np.zeros(shape, np.uint64), np.zeros(shape, np.uint64)
        k32 = np.zeros(1, np.int32)
        self.eng._check(self._L.bh_posterior_column_quantiles(self._p, dep.size, _ptr(dep), rank.shape[1], _ptr(rank), _ptr(lo),
                                                              _ptr(up), _ptr(k32)))
        return lo, up, bool(k32[0])

    def hist(self, dep, dbin, nd, edges_per_site, argmax=False):
        dep = np.ascontiguousarray(dep, np.float64)
        dbin = np.ascontiguousarray(dbin, np.int32)
        nb = np.array([e.size - 1 for e in edges_per_site], np.int64)
        edge_off = np.concatenate(([0], np.cumsum(nb + 1))).astype(np.int64)
        edges = np.ascontiguousarray(np.concatenate(edges_per_site), np.float64)
        counts = np.zeros(int(np.sum(nb * nd)), np.uint32)
        am = np.zeros((self.S, nd), np.int32) if argmax else None
        self.eng._check(self._L.bh_posterior_hist(self._p, dep.size, _ptr(dep), _ptr(dbin), int(nd), _ptr(edge_off),
                                                  _ptr(edges), _ptr(counts), _ptr(am)))
        off = np.concatenate(([0], np.cumsum(nb * nd)))
        return [counts[off[s]:off[s + 1]].reshape(nb[s], nd) for s in range(self.S)], am

    def interfaces(self, edges):
        edges = np.ascontiguousarray(edges, np.float64)
        counts = np.zeros((self.S, edges.size - 1), np.uint32)
        self.eng._check(self._L.bh_posterior_interfaces(self._p, edges.size, _ptr(edges), _ptr(counts)))
        return counts

    # ---- scalar sets (include/bh_engine_posterior_scalars.h) ----

    def moho(self, lo, hi, mohovs):
        lo, hi, mohovs = (np.ascontiguousarray(v, np.float64) for v in (lo, hi, mohovs))
        found = np.zeros(self.S, np.int64)
        self.eng._check(self._L.bh_posterior_moho(self._p, _ptr(lo), _ptr(hi), _ptr(mohovs), _ptr(found)))
        return found

    def attach(self, values, nlayers):
        """values: None or a 2-D float32/float64 array or device tensor, one value row per loaded input row"""
        if values is None:
            self.eng._check(self._L.bh_posterior_attach(self._p, E.HOST, None, 8, 0, 0, None, int(bool(nlayers))))
            return
        if isinstance(values, np.ndarray):
            values = np.ascontiguousarray(values)
            mem, stream, ptr = E.HOST, None, _ptr(values)
            ld, elem = values.shape[1], values.itemsize
        else:
            import torch
            if values.stride(1) != 1:
                values = values.contiguous()
            mem, stream = E.DEVICE, C.c_void_p(torch.cuda.current_stream(values.device).cuda_stream)
            ptr, ld, elem = C.c_void_p(values.data_ptr()), values.stride(0), values.element_size()
        if values.shape[0] != self.N:
            raise ValueError("one value row per model row")
        self.eng._check(self._L.bh_posterior_attach(self._p, mem, stream, elem, values.shape[1], ld, ptr, int(bool(nlayers))))

    def features(self, kinds, par):
        """bh_posterior_features: kinds int32 [F], par float64 [S, F, 3] (check_features) -> found int64 [S, ncols]"""
        kinds = np.ascontiguousarray(kinds, np.int32)
        par = np.ascontiguousarray(par, np.float64)
        if par.shape != (self.S, kinds.size, 3):
            raise ValueError("par must be [nsites][F][3]")
        if kinds.size and not (0 <= kinds.min() and kinds.max() < len(FEATURE_KINDS)):
            raise ValueError("kinds must be BH_FEATURE_* numbers")
        found = np.zeros((self.S, sum(FEATURE_COLS[FEATURE_KINDS[k]] for k in kinds)), np.int64)
        self.eng._check(self._L.bh_posterior_features(self._p, kinds.size, _ptr(kinds), _ptr(par), _ptr(found)))
        return found

    def classes(self, K, term_class, term_set, term_col, term_op, lo, hi, device=None):
        """bh_posterior_classes -> (cls int32 [N]: a numpy array, or a tensor on `device` where given; counts int64 [S, K + 1])"""
        tc, ts, tq, to = (np.ascontiguousarray(v, np.int32) for v in (term_class, term_set, term_col, term_op))
        T = tc.size
        lo, hi = (np.ascontiguousarray(v, np.float64).reshape(self.S, T) for v in (lo, hi))
        counts = np.zeros((self.S, K + 1), np.int64)
        if device is None:
            cls = np.zeros(self.N, np.int32)
            mem, stream, ptr = E.HOST, None, _ptr(cls)
        else:
            import torch
            cls = torch.empty(self.N, dtype=torch.int32, device=device)
            mem, stream, ptr = E.DEVICE, C.c_void_p(torch.cuda.current_stream(device).cuda_stream), C.c_void_p(cls.data_ptr())
        self.eng._check(self._L.bh_posterior_classes(self._p, int(K), T, _ptr(tc), _ptr(ts), _ptr(tq), _ptr(to), _ptr(lo), _ptr(hi),
                                                     mem, stream, ptr, _ptr(counts)))
        return cls, counts

    def export(self, which, device=None):
        """bh_posterior_scalar_export: the set's columns by input row, float64 [N, Q] (NaN for a row the load left out): a numpy
        array, or a tensor on `device` where given"""
        q = np.zeros(1, np.int32)
        self.eng._check(self._L.bh_posterior_scalar_cols(self._p, which, _ptr(q)))
        Q = int(q[0])
        if device is None:
            out = np.zeros((self.N, Q))
            mem, stream, ptr = E.HOST, None, _ptr(out)
        else:
            import torch
            out = torch.empty((self.N, Q), dtype=torch.float64, device=device)
            mem, stream, ptr = E.DEVICE, C.c_void_p(torch.cuda.current_stream(device).cuda_stream), C.c_void_p(out.data_ptr())
        self.eng._check(self._L.bh_posterior_scalar_export(self._p, which, mem, stream, Q, ptr))
        return out

    def gather(self, which, pos, Q):
        """the values [len(pos), Q] of the loaded rows at the positions pos of a set of Q columns (bh_posterior_scalar_gather)"""
        pos = np.ascontiguousarray(pos, np.int64)
        out = np.zeros((pos.size, Q))
        self.eng._check(self._L.bh_posterior_scalar_gather(self._p, which, pos.size, _ptr(pos), _ptr(out)))
        return out

    def scalar_stats(self, which, median=True):
        q = np.zeros(1, np.int32)
        self.eng._check(self._L.bh_posterior_scalar_cols(self._p, which, _ptr(q)))
        S, Q = self.S, int(q[0])
        out = dict(count=np.zeros((S, Q), np.int64), nan=np.zeros((S, Q), np.int64), kmin=np.zeros((S, Q), np.uint64),
                   kmax=np.zeros((S, Q), np.uint64), scale=np.zeros((S, Q), np.int32), x0=np.zeros((S, Q), np.int64),
                   exact=np.zeros((S, Q), np.int32), sums=np.zeros((S, Q, 6), np.uint64),
                   median=np.zeros((S, Q, 2), np.uint64) if median else None)
        self.eng._check(self._L.bh_posterior_scalar_stats(self._p, which, _ptr(out["count"]), _ptr(out["nan"]), _ptr(out["kmin"]),
                                                          _ptr(out["kmax"]), _ptr(out["scale"]), _ptr(out["x0"]),
                                                          _ptr(out["exact"]), _ptr(out["sums"]), _ptr(out["median"])))
        out["min"] = _keys_to_values(out["kmin"], False).reshape(S, Q)
        out["max"] = _keys_to_values(out["kmax"], False).reshape(S, Q)
        if median:
            out["med"] = _keys_to_values(out["median"].reshape(-1), False).reshape(S, Q, 2)
        return out

    def quantile_keys(self, which, rank):
        """rank uint32 [S, Q, R] -> (lower, upper) uint64 keys [S, Q, R]: the order statistics rank and rank + 1 of a set's columns"""
        rank = np.ascontiguousarray(rank, np.uint32)
        lo, up = np.zeros(rank.shape, np.uint64), np.zeros(rank.shape, np.uint64)
        self.eng._check(self._L.bh_posterior_scalar_quantiles(self._p, which, rank.shape[2], _ptr(rank), _ptr(lo), _ptr(up)))
        return lo, up

    def cov(self, dep, which=-1, cols=(), finished=True):
        """bh_posterior_cov of the vs at dep and the columns cols of the set `which` (include/bh_engine_posterior_cov.h): a dict of
        n, masked [S], L, x0, exact, s [S, P], raw [S, P (P + 1) / 2, 3] and, with finished, mean [S, P], cov, corr [S, P, P]"""
        dep = np.ascontiguousarray(dep, np.float64)
        cols = np.ascontiguousarray(cols, np.int32)
        S, P = self.S, dep.size + cols.size
        out = dict(n=np.zeros(S, np.int64), masked=np.zeros(S, np.int64), L=np.zeros((S, P), np.int32), x0=np.zeros((S, P), np.int64),
                   exact=np.zeros((S, P), np.int32), s=np.zeros((S, P), np.uint64), raw=np.zeros((S, P * (P + 1) // 2, 3), np.uint64))
        if finished:
            out.update(mean=np.zeros((S, P)), cov=np.zeros((S, P, P)), corr=np.zeros((S, P, P)))
        self.eng._check(self._L.bh_posterior_cov(self._p, dep.size, _ptr(dep), int(which), cols.size, _ptr(cols), _ptr(out["n"]),
                                                 _ptr(out["masked"]), _ptr(out["L"]), _ptr(out["x0"]), _ptr(out["exact"]), _ptr(out["s"]),
                                                 _ptr(out["raw"]), _ptr(out.get("mean")), _ptr(out.get("cov")), _ptr(out.get("corr"))))
        return out

    @staticmethod
    def _edges(edges_per_site):
        nb = np.array([len(e) - 1 for e in edges_per_site], np.int64)
        off = np.concatenate(([0], np.cumsum(nb + 1))).astype(np.int64)
        return nb, off, np.ascontiguousarray(np.concatenate([np.asarray(e, np.float64) for e in edges_per_site]), np.float64)

    def scalar_hist(self, which, col, edges_per_site):
        nb, off, edges = self._edges(edges_per_site)
        counts = np.zeros(int(nb.sum()), np.uint32)
        self.eng._check(self._L.bh_posterior_scalar_hist(self._p, which, int(col), _ptr(off), _ptr(edges), _ptr(counts)))
        co = np.concatenate(([0], np.cumsum(nb)))
        return [counts[co[s]:co[s + 1]] for s in range(self.S)]

    def scalar_hist2d(self, which, colx, coly, xedges_per_site, yedges_per_site, argmax=True):
        nx, xoff, xe = self._edges(xedges_per_site)
        ny, yoff, ye = self._edges(yedges_per_site)
        counts = np.zeros(int(np.sum(nx * ny)), np.uint32)
        am = np.zeros(self.S, np.int64) if argmax else None
        self.eng._check(self._L.bh_posterior_scalar_hist2d(self._p, which, int(colx), int(coly), _ptr(xoff), _ptr(xe), _ptr(yoff),
                                                           _ptr(ye), _ptr(counts), _ptr(am)))
        co = np.concatenate(([0], np.cumsum(nx * ny)))
        return [counts[co[s]:co[s + 1]].reshape(nx[s], ny[s]) for s in range(self.S)], am


def _mean_std(n, sums, scale, x0):
    """mean and population std of one column from its exact integer sums (include/bh_engine_posterior.h)."""
    s = [int(v) for v in sums]
    S1 = s[0] + (s[1] << 32)
    S2 = s[2] + (s[3] << 32) + (s[4] << 64) + (s[5] << 96)
    L, X0 = int(scale), int(x0)
    num = S1 + n * X0                                   # sum(v) * 2^-L
    mean = (num << L) / n if L >= 0 else num / (n << -L)  # int / int: correctly rounded
    V = n * S2 - S1 * S1                                # n^2 var * 2^-2L, >= 0
    if V == 0:
        return mean, 0.0
    k = max(0, (120 - V.bit_length()) // 2 + 1)
    q = math.isqrt(V << (2 * k))                        # floor(sqrt(V) * 2^k), >= 2^60
    e = L - k
    std = (q << e) / n if e >= 0 else q / (n << -e)
    return mean, std


def _site_groups(misfits, site, N):
    if misfits is None:
        return None
    try:
        import torch
        if isinstance(misfits, torch.Tensor):
            misfits = misfits.detach().cpu().numpy()
        if isinstance(site, torch.Tensor):
            site = site.detach().cpu().numpy()
    except ImportError:
        pass
    misfits = np.asarray(misfits, np.float64).reshape(-1)
    if misfits.size != N:
        raise ValueError("one misfit per row")
    return misfits, (np.zeros(N, np.int64) if site is None else np.asarray(site).astype(np.int64))


def _row(models, i):
    r = models[i]
    if hasattr(r, "detach"):
        r = r.detach().cpu().numpy()
    return np.asarray(r)


def posterior_models(models, site=None, dep_int=None, misfits=None, engine=None, nsites=None, quantiles=None, classes=None):
    """get_singlemodels of every site: a list of dicts (one dict when site is None).  Keys: mean, median, minmax,
    stdminmax (each (values, dep_int)), mode ((vs_mode, dep_center); NaN and mode_valid False where the reference raises,
    i.e. the site's vs range is below one 0.025 km/s bin), minmisfit (with misfits), count, mode_valid, invalid_rows.
    quantiles: a sequence of numbers in [0, 1] (any order, duplicates allowed; anything else is a ValueError) adds the keys
    quantiles = (values [R, D], dep_int) and q (the requested quantiles, float64): values[i, j] is numpy.quantile(column j, q[i],
    method="linear") of the site's float64 column of interpolated vs -- the credible band of vs against depth -- NaN for a site
    without rows (include/bh_engine_posterior_quantiles.h; the columns are never stored).  quantiles at 0.5 need not equal
    `median` in the last bit for an even count: median is (a + b) / 2, numpy's quantile b - (b - a) * 0.5, of the same two
    order statistics a <= b.
    classes: the dict posterior_classes returned for the same rows: the result is then per site a dict class name -> the dict
    described here, of the rows of that class alone (posterior_classes says how rows in no class are accounted for)."""
    if classes is not None:
        return _by_class(posterior_models, classes, models, site, dict(dep_int=dep_int, misfits=misfits, engine=engine, nsites=nsites,
                                                                       quantiles=quantiles))
    qs = check_quantiles(quantiles)
    dep = default_dep_int() if dep_int is None else np.ascontiguousarray(dep_int, np.float64)
    ld = _Loaded(models, site, engine, nsites)
    try:
        qv = column_quantiles(ld, dep, qs) if qs is not None else None
        col = ld.columns(dep, median=True)
        S, D = ld.S, dep.size
        vmin_s = np.array([col["min"][s].min() if ld.rows[s] else np.nan for s in range(S)])
        vmax_s = np.array([col["max"][s].max() if ld.rows[s] else np.nan for s in range(S)])
        nbins = np.zeros(S, np.int64)
        edges = []
        for s in range(S):
            if ld.rows[s]:
                nbins[s] = int((vmax_s[s] - vmin_s[s]) / VS_INTERVAL)
        if int(np.sum(nbins)) * (D - 1) > MAX_COUNTS:   # (before numpy builds the edges of a wild range)
            raise E.EngineError("engine call failed (%d): the mode histogram would hold %d cells, above "
                                "BH_POSTERIOR_MAXCOUNTS (%d): is the vs range sane?" % (E.BH_EINVAL, int(np.sum(nbins)) * (D - 1), MAX_COUNTS))
        for s in range(S):
            edges.append(np.linspace(vmin_s[s], vmax_s[s], nbins[s] + 1) if nbins[s] > 0 else np.array([0.0, 1.0]))
        dbin = depth_bins(dep, dep)
        _, am = ld.hist(dep, dbin, D - 1, edges, argmax=True)
        med = _keys_to_values(col["median"].reshape(-1), col["keys32"]).reshape(S, D, 2)
    finally:
        ld.close()
    groups = _site_groups(misfits, site, ld.N)
    dep_center = (dep[:-1] + dep[1:]) / 2.
    out = []
    for s in range(S):
        n = int(ld.rows[s])
        r = dict(count=n, invalid_rows=int(ld.invalid[s]), mode_valid=bool(nbins[s] > 0))
        if n:
            ms = [_mean_std(n, col["sums"][s, j], col["scale"][s, j], col["x0"][s, j]) for j in range(D)]
            mean = np.array([m for m, _ in ms])
            std = np.array([v for _, v in ms])
            lo, hi = med[s, :, 0], med[s, :, 1]
            median = (lo + hi) / 2. if n % 2 == 0 else lo.copy()
            vmin, vmax = col["min"][s], col["max"][s]
        else:
            mean = std = median = vmin = vmax = np.full(D, np.nan)
        r["mean"] = (mean, dep)
        r["median"] = (median, dep)
        r["minmax"] = (np.array((vmin, vmax)), dep)
        r["stdminmax"] = (np.array((mean - std, mean + std)), dep)
        if r["mode_valid"]:
            e = edges[s]
            vs_center = (e[:-1] + e[1:]) / 2.
            r["mode"] = (vs_center[am[s]], dep_center)
        else:
            r["mode"] = (np.full(D - 1, np.nan), dep_center)
        if qs is not None:
            r["quantiles"] = (qv[s], dep)
            r["q"] = qs.copy()
        if groups is not None:
            mis, sidx = groups
            idx = np.flatnonzero(sidx == s)
            if idx.size:
                r["minmisfit"] = stepmodel(_row(models, idx[np.argmin(mis[idx])]))
        out.append(r)
    return out[0] if site is None else out


def posterior_hist2d(models, site=None, dep_int=None, vs_edges=None, dep_edges=None, engine=None, nsites=None, classes=None):
    """The 2-D posterior plot's numbers (_plot_bestmodels_hist) of every site: a list of dicts (one dict when site is
    None) with counts [nvs, ndep] of the vs sampled at `samples` over vs_edges x dep_edges (numpy.histogram2d), and
    interfaces [ndep] = numpy.histogram of the interface depths over dep_edges.  The defaults are the plot's
    (hist2d_edges): dep_int None -> 0.5 km sampling of 0..100 km and 1 km depth bins; vs edges from each site's range.
    classes: the dict posterior_classes returned for the same rows: the result is then per site a dict class name -> the dict
    described here, of the rows of that class alone (posterior_classes says how rows in no class are accounted for)."""
    if classes is not None:
        return _by_class(posterior_hist2d, classes, models, site, dict(dep_int=dep_int, vs_edges=vs_edges, dep_edges=dep_edges,
                                                                       engine=engine, nsites=nsites))
    samples, depbins, _ = hist2d_edges(None, None, dep_int)
    if dep_edges is not None:
        depbins = np.asarray(dep_edges, np.float64)
    ld = _Loaded(models, site, engine, nsites)
    try:
        S = ld.S
        if vs_edges is None:
            col = ld.columns(samples, median=False)
            vs_e = []
            for s in range(S):
                if not ld.rows[s]:
                    vs_e.append(np.array([0.0, 1.0]))
                    continue
                vs_e.append(hist2d_edges(col["min"][s].min(), col["max"][s].max(), dep_int)[2])
        else:
            vs_e = [np.asarray(vs_edges, np.float64)] * S
        counts, _ = ld.hist(samples, depth_bins(samples, depbins), depbins.size - 1, vs_e)
        inter = ld.interfaces(depbins)
    finally:
        ld.close()
    out = [dict(counts=counts[s], vs_edges=vs_e[s], dep_edges=depbins, samples=samples, interfaces=inter[s],
                count=int(ld.rows[s]), invalid_rows=int(ld.invalid[s])) for s in range(S)]
    return out[0] if site is None else out


# ---- Moho depth, crustal velocity and scalar columns (include/bh_engine_posterior_scalars.h) ----------------------------

MOHO_COLUMNS = ("moho", "vslast", "vscrust", "vsjump")
MOHOVS = 4.2  # km/s: the reference's default of the vs that marks the mantle


def moho_edges(vmin, vmax, bins=50):
    """The float64 edges matplotlib's hist / hist2d (numpy.histogram, numpy.histogram2d) form for data of that min and max:
    `bins` equal bins over [min, max], [min - 0.5, max + 0.5] where they are equal, [0, 1] where there is no data."""
    if vmin is None or np.isnan(vmin):
        return np.histogram_bin_edges(np.zeros(0), bins)
    return np.histogram_bin_edges(np.array([vmin, vmax], np.float64), bins)


def scalar_edges(vmin, vmax, dtype, bins=20, nlayers=False):
    """The edges of the reference's scalar posterior plots (_plot_posterior_distribution) for a column of that dtype, min
    and max: numpy.histogram_bin_edges of the data; for nlayers arange(min, max + 2) - 0.5; for a constant column the
    reference's placeholder [m - 1, m - 0.1, m + 0.1, m + 1]; [0, 1] where there is no data."""
    if vmin is None or np.isnan(vmin):
        return np.histogram_bin_edges(np.zeros(0, dtype), bins)
    if nlayers:
        return np.arange(vmin, vmax + 2) - 0.5
    if vmin == vmax:
        m = float(vmin)
        return np.array([m - 1, m - 0.1, m + 0.1, m + 1])
    return np.histogram_bin_edges(np.array([vmin, vmax], dtype), bins)


def median_of_middles(a, b, n, dtype=np.float64):
    """numpy.median of n values whose two middle ones (ranks (n-1)//2 and (n-1)//2 + 1) are a and b, in `dtype`."""
    a, b = dtype(a), dtype(b)
    if n % 2:
        return a
    with np.errstate(over="ignore"):
        return (a + b) / dtype(2)


def _per_site(v, S, width, what):
    v = np.asarray(v, np.float64)
    if v.shape == (width,) or v.shape == ():
        v = np.broadcast_to(v, (S,) + v.shape)
    if v.shape != ((S, width) if width else (S,)):
        raise ValueError("%s: one %s or one per site" % (what, "pair" if width else "value"))
    return np.ascontiguousarray(v)


def _stat_dict(st, s, q, dtype=np.float64):
    n = int(st["count"][s, q])
    if not n:
        return dict(median=np.nan, mean=np.nan, std=np.nan, min=np.nan, max=np.nan)
    mean, std = _mean_std(n, st["sums"][s, q], st["scale"][s, q], st["x0"][s, q])
    return dict(median=median_of_middles(st["med"][s, q, 0], st["med"][s, q, 1], n, dtype), mean=mean, std=std,
                min=dtype(st["min"][s, q]), max=dtype(st["max"][s, q]))


def posterior_moho(models, site=None, moho=None, mohovs=MOHOVS, bins=50, engine=None, nsites=None, quantiles=None, classes=None):
    """The numbers of the reference's plot_moho_crustvel_tradeoff for every site: a list of dicts (one dict when site is
    None).  moho = (lo, hi) km, or one pair per site: the depth range in which an interface can be the Moho (0 <= lo < hi);
    mohovs (one, or one per site): the Moho is the first interface inside the range below which vs exceeds it.
    Keys: rows, count (the rows with a Moho), invalid_rows, dropped (device rows with a site index out of range, e.g. -1:
    left out; the total of the call); moho, vslast (vs of the last crustal layer), vscrust (the mean
    crustal vs above the Moho), vsjump (the vs step at the Moho): each a dict of median, mean, std, min, max; hist: name ->
    (counts [bins], edges); hist2d: vslast / vscrust / vsjump -> (counts [bins, bins], xedges, yedges) against moho; mode:
    the same names -> (x, y), the centres of the first largest cell.  A site without a Moho row has count 0, NaN statistics
    and empty histograms over [0, 1].
    quantiles: a sequence of numbers in [0, 1] (any order, duplicates allowed; anything else is a ValueError) adds to each of the
    four dicts quantiles [R] = numpy.quantile(values, quantiles, method="linear") over the rows that have a Moho -- the credible
    interval of the Moho depth -- NaN where count is 0.  quantiles at 0.5 need not equal median
    in the last bit for an even count ((a + b) / 2 against numpy's b - (b - a) * 0.5 of the same two order statistics).
    classes: the dict posterior_classes returned for the same rows: the result is then per site a dict class name -> the dict
    described here, of the rows of that class alone (posterior_classes says how rows in no class are accounted for)."""
    if classes is not None and moho is not None:
        return _by_class(posterior_moho, classes, models, site, dict(moho=moho, mohovs=mohovs, bins=bins, engine=engine, nsites=nsites,
                                                                     quantiles=quantiles))
    qs = check_quantiles(quantiles)
    if moho is None:
        raise ValueError("moho=(lo, hi) is needed: the reference's default is the station's priors['z']")
    ld = _Loaded(models, site, engine, nsites, scalars=True)
    try:
        S = ld.S
        rng = _per_site(moho, S, 2, "moho")
        mv = _per_site(mohovs, S, 0, "mohovs")
        found = ld.moho(rng[:, 0], rng[:, 1], mv)
        st = ld.scalar_stats(E.SCALARS_MOHO)
        qv = set_quantiles(ld, E.SCALARS_MOHO, st["count"], qs) if qs is not None else None
        edges = [[moho_edges(st["min"][s, q], st["max"][s, q], bins) if found[s] else moho_edges(None, None, bins)
                  for s in range(S)] for q in range(4)]
        h1 = [ld.scalar_hist(E.SCALARS_MOHO, q, edges[q]) for q in range(4)]
        h2 = [ld.scalar_hist2d(E.SCALARS_MOHO, q, 0, edges[q], edges[0]) for q in (1, 2, 3)]
    finally:
        ld.close()
    out = []
    for s in range(S):
        r = dict(rows=int(ld.rows[s]), count=int(found[s]), invalid_rows=int(ld.invalid[s]), dropped=ld.dropped, hist={}, hist2d={},
                 mode={})
        for q, name in enumerate(MOHO_COLUMNS):
            r[name] = _stat_dict(st, s, q)
            if qs is not None:
                r[name]["quantiles"] = qv[s, q].copy()
            r["hist"][name] = (h1[q][s].astype(np.int64), edges[q][s])
        for i, q in enumerate((1, 2, 3)):
            name = MOHO_COLUMNS[q]
            counts, am = h2[i]
            xe, ye = edges[q][s], edges[0][s]
            r["hist2d"][name] = (counts[s].astype(np.int64), xe, ye)
            if found[s]:
                xi, yi = divmod(int(am[s]), ye.size - 1)
                r["mode"][name] = (((xe[:-1] + xe[1:]) / 2.)[xi], ((ye[:-1] + ye[1:]) / 2.)[yi])
            else:
                r["mode"][name] = (np.nan, np.nan)
        out.append(r)
    return out[0] if site is None else out


def _stack_columns(columns, N):
    """(values [N, Q] or None, [(name, index or None, numpy dtype)]): the columns side by side in one array or device tensor"""
    try:
        import torch
    except ImportError:
        torch = None
    parts, layout = [], []
    for name, v in columns.items():
        is_t = torch is not None and isinstance(v, torch.Tensor)
        if is_t:
            if v.dtype not in (torch.float32, torch.float64):
                raise ValueError("column %r must be float32 or float64" % name)
            dt = np.float32 if v.dtype == torch.float32 else np.float64
        else:
            v = np.asarray(v)
            if v.dtype not in (np.float32, np.float64):
                v = v.astype(np.float64)
            dt = v.dtype.type
        if v.ndim not in (1, 2) or v.shape[0] != N:
            raise ValueError("column %r must be [N] or [N, k] with one row per model row" % name)
        if v.ndim == 1:
            layout.append((name, None, dt))
            parts.append(v[:, None])
        else:
            layout += [(name, i, dt) for i in range(v.shape[1])]
            parts.append(v)
    if not parts:
        return None, layout
    if len(layout) > 64:
        raise ValueError("at most 64 scalar columns in one call (BH_SCALARS_MAXCOLS)")
    wide = any(dt is np.float64 for _, _, dt in layout)
    tens = [p for p in parts if not isinstance(p, np.ndarray)]
    if tens:   # any device column: all of them on the device (float32 widens exactly)
        tdt = torch.float64 if wide else torch.float32
        parts = [(torch.from_numpy(np.ascontiguousarray(p)) if isinstance(p, np.ndarray) else p).to(device=tens[0].device, dtype=tdt)
                 for p in parts]
        return (parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)), layout
    ndt = np.float64 if wide else np.float32
    return np.concatenate([p.astype(ndt, copy=False) for p in parts], axis=1), layout


def posterior_scalars(models, columns, site=None, bins=20, nlayers=True, engine=None, nsites=None, quantiles=None, classes=None):
    """The numbers of the reference's plot_posterior_likes / _misfits / _nlayers / _vpvs / _noise / _others for every site: a
    list of dicts (one dict when site is None), name -> statistics.  columns: a dict name -> [N] or [N, k] values (float32 or
    float64; numpy arrays or device tensors), one row per model row; a [N, k] column gives a list of k statistics.  With
    nlayers, the key "nlayers" holds the number of layers n - 1 of the rows.  Statistics: median (numpy's for the column's
    dtype), mean, std, min, max, count, nan (the rows whose value is NaN: they are left out of this column only), constant,
    hist = (counts, edges) and mode (the centre of the first largest bin).  Edges are numpy.histogram_bin_edges(data, bins) in
    the column's dtype; nlayers has the reference's arange(min, max + 2) - 0.5.  constant = (min == max): the column gets the
    reference's placeholder edges [m - 1, m - 0.1, m + 0.1, m + 1].  (The reference tests np.std(data) == 0 instead, which
    numpy's own rounding of the mean can miss on a constant column; min == max cannot.)  The dict also holds rows,
    invalid_rows and dropped (as posterior_moho); a column of one of these names, or "nlayers" beside the built-in one, is a
    ValueError.
    quantiles: a sequence of numbers in [0, 1] (any order, duplicates allowed; anything else is a ValueError) adds to every
    column's statistics, nlayers included, quantiles [R] float64 = numpy.quantile(values widened to float64, quantiles,
    method="linear") over the column's non-NaN values, NaN where count is 0 -- whatever the column's dtype (numpy computes a
    float32 column's quantile in float32; median keeps its per-dtype meaning).  quantiles at 0.5 need not equal median in the
    last bit for an even count ((a + b) / 2 against numpy's b - (b - a) * 0.5 of the same two order statistics).
    classes: the dict posterior_classes returned for the same rows: the result is then per site a dict class name -> the dict
    described here, of the rows of that class alone (posterior_classes says how rows in no class are accounted for)."""
    if classes is not None:
        return _by_class(posterior_scalars, classes, models, site, dict(columns=columns, bins=bins, nlayers=nlayers, engine=engine,
                                                                        nsites=nsites, quantiles=quantiles))
    qs = check_quantiles(quantiles)
    taken = [k for k in columns if k in ("rows", "invalid_rows", "dropped") or (nlayers and k == "nlayers")]
    if taken:
        raise ValueError("column name %r is a key of the result itself: give the column another name" % (taken[0],))
    ld = _Loaded(models, site, engine, nsites, scalars=True)
    try:
        S = ld.S
        values, layout = _stack_columns(columns, ld.N)
        if nlayers:
            layout = layout + [("nlayers", None, np.float64)]
        if not layout:
            raise ValueError("no column and no nlayers: nothing to summarise")
        ld.attach(values, nlayers)
        st = ld.scalar_stats(E.SCALARS_USER)
        qv = set_quantiles(ld, E.SCALARS_USER, st["count"], qs) if qs is not None else None
        Q = len(layout)
        edges = [[scalar_edges(st["min"][s, q], st["max"][s, q], layout[q][2], bins, nlayers and q == Q - 1)
                  if st["count"][s, q] else scalar_edges(None, None, layout[q][2], bins) for s in range(S)] for q in range(Q)]
        hists = [ld.scalar_hist(E.SCALARS_USER, q, edges[q]) for q in range(Q)]
    finally:
        ld.close()
    out = []
    for s in range(S):
        r = dict(rows=int(ld.rows[s]), invalid_rows=int(ld.invalid[s]), dropped=ld.dropped)
        for q, (name, idx, dt) in enumerate(layout):
            d = _stat_dict(st, s, q, dt)
            n = int(st["count"][s, q])
            e = edges[q][s]
            cnt = hists[q][s].astype(np.int64)
            d.update(count=n, nan=int(st["nan"][s, q]), constant=bool(n and st["min"][s, q] == st["max"][s, q]), hist=(cnt, e),
                     mode=((e[:-1] + e[1:]) / 2.)[np.argmax(cnt)] if n else np.nan)
            if qs is not None:
                d["quantiles"] = qv[s, q].copy()
            if idx is None:
                r[name] = d
            else:
                r.setdefault(name, []).append(d)
        out.append(r)
    return out[0] if site is None else out


# ---- covariance and correlation of vs with depth (include/bh_engine_posterior_cov.h) ---------------------------------------

def posterior_covariance(models, site=None, dep_int=None, columns=None, moho=None, mohovs=MOHOVS, moho_columns=("moho", "vscrust"),
                         engine=None, nsites=None, features=None, classes=None):
    """How a site's profile varies together: a list of dicts (one dict when site is None) with the mean vector and the
    population covariance (ddof = 0, as std everywhere in this package) and correlation matrices of P columns -- the vs at the
    depths of dep_int (default 0..100 km in 0.5 km steps; an empty dep_int leaves them out), then scalar columns of ONE set:
    columns: as posterior_scalars', name -> [N] or [N, k] values, one row per model row (a [N, k] column gives the labels
      name[0] .. name[k-1]); or
    moho = (lo, hi) km, or one pair per site, with mohovs: as posterior_moho's -- the columns named by moho_columns (of moho,
      vslast, vscrust, vsjump) are appended; or
    features: as posterior_features', name -> (kind, z0, z1[, c]) -- every feature's columns are appended under the labels name,
      or name.value / name.depth / name.jump for the kinds of two columns.
    Two of columns, moho and features together is a ValueError: one call takes its scalar columns from one set.  A row with NaN
    in any of the scalar columns (a row without a Moho, without the drop asked for) is left out of the whole matrix (listwise
    deletion: the matrix stays a covariance).
    Keys: dep, names (the P labels: the depths, then the column names), n (the rows used), masked (the rows left out), mean [P],
    std [P] (the square root of cov's diagonal), cov [P, P], corr [P, P], exact [P] (bool: the column's values went into the
    integer sums without rounding).  corr is NaN in the row and column of a constant column, as numpy.corrcoef leaves it; a site
    without rows used has NaN everywhere.  The numbers are functions of exact integer sums formed on the device: the same bits
    alone or among other sites, in any row order, on every repeat; each within 1 ulp of the exact rational.  The caller who wants
    ddof = 1 multiplies cov by n / (n - 1).
    classes: the dict posterior_classes returned for the same rows: the result is then per site a dict class name -> the dict
    described here, of the rows of that class alone (posterior_classes says how rows in no class are accounted for)."""
    if classes is not None:
        return _by_class(posterior_covariance, classes, models, site, dict(dep_int=dep_int, columns=columns, moho=moho, mohovs=mohovs,
                                                                           moho_columns=moho_columns, engine=engine, nsites=nsites,
                                                                           features=features))
    if sum(v is not None for v in (columns, moho, features)) > 1:
        raise ValueError("one call takes its scalar columns from one set: give columns, moho or features, not two of them")
    dep = default_dep_int() if dep_int is None else np.ascontiguousarray(dep_int, np.float64).reshape(-1)
    if moho is not None:
        bad = [c for c in moho_columns if c not in MOHO_COLUMNS]
        if bad or not len(moho_columns):
            raise ValueError("moho_columns must name some of %r" % (MOHO_COLUMNS,))
    ld = _Loaded(models, site, engine, nsites, scalars=columns is not None or moho is not None or features is not None)
    try:
        S = ld.S
        which, cols, names = -1, [], []
        if features is not None:
            kinds, par, names = check_features(features, S)
            ld.features(kinds, par)
            which, cols = E.SCALARS_FEATURES, list(range(len(names)))
        elif columns is not None:
            values, layout = _stack_columns(columns, ld.N)
            if values is not None:
                ld.attach(values, False)
                which, cols = E.SCALARS_USER, list(range(len(layout)))
                names = [name if idx is None else "%s[%d]" % (name, idx) for name, idx, _ in layout]
        elif moho is not None:
            rng = _per_site(moho, S, 2, "moho")
            ld.moho(rng[:, 0], rng[:, 1], _per_site(mohovs, S, 0, "mohovs"))
            which, cols, names = E.SCALARS_MOHO, [MOHO_COLUMNS.index(c) for c in moho_columns], list(moho_columns)
        P = dep.size + len(cols)
        if not 1 <= P <= E.COV_MAXCOLS:
            raise ValueError("%d columns: a call takes 1 .. %d (BH_COV_MAXCOLS)" % (P, E.COV_MAXCOLS))
        r = ld.cov(dep, which, cols)
    finally:
        ld.close()
    labels = [float(d) for d in dep] + names
    out = []
    for s in range(S):
        with np.errstate(invalid="ignore"):
            std = np.sqrt(np.diagonal(r["cov"][s]))
        out.append(dict(dep=dep, names=list(labels), n=int(r["n"][s]), masked=int(r["masked"][s]), mean=r["mean"][s].copy(), std=std,
                        cov=r["cov"][s].copy(), corr=r["corr"][s].copy(), exact=r["exact"][s] != 0))
    return out[0] if site is None else out


# ---- structural features of the layered models (include/bh_engine_posterior_features.h) ------------------------------------

FEATURE_KINDS = ("vsmean", "vstime", "tts", "vsmin", "vsmax", "drop", "jump", "above", "nifaces")   # BH_FEATURE_*, in order
FEATURE_COLS = dict(vsmean=1, vstime=1, tts=1, vsmin=2, vsmax=2, drop=2, jump=2, above=1, nifaces=1)
FEATURE_PARTS = dict(vsmin=("value", "depth"), vsmax=("value", "depth"), drop=("depth", "jump"), jump=("depth", "jump"))
FEATURE_OPTIONAL = ("drop", "jump", "above")   # a row may lack them: they carry a probability
_RESULT_KEYS = ("rows", "invalid_rows", "dropped")


def check_features(features, S):
    """The user's dict name -> (kind, z0, z1[, c]) as (kinds int32 [F], par float64 [S, F, 3], labels [ncols]) for
    bh_posterior_features over S sites.  kind is one of FEATURE_KINDS; z0 < z1 (km) is the depth window; c is the threshold of
    drop and jump (km/s, >= 0, default 0) and the velocity of above (needed there); the other kinds take no c.  Every number is a
    scalar or a sequence of one value per site.  labels: the name for a kind of one column, name.value, name.depth (vsmin,
    vsmax) or name.depth, name.jump (drop, jump) for a kind of two.  Pure host code; every refused input is a ValueError that names
    the feature (and the site, where one site's value is at fault)."""
    if not isinstance(features, dict) or not features:
        raise ValueError("features must be a dict name -> (kind, z0, z1[, c]) with at least one entry")
    if len(features) > E.FEATURES_MAXKINDS:
        raise ValueError("features: %d features, a call takes at most %d" % (len(features), E.FEATURES_MAXKINDS))
    S = int(S)
    kinds, labels = [], []
    par = np.zeros((S, len(features), 3))
    for f, (name, spec) in enumerate(features.items()):
        if not isinstance(name, str) or not name:
            raise ValueError("feature %r: the name must be a non-empty string" % (name,))
        if name in _RESULT_KEYS:
            raise ValueError("feature %r: the name is a key of the result itself: give the feature another name" % (name,))
        if isinstance(spec, (str, bytes)) or not hasattr(spec, "__len__") or len(spec) not in (3, 4):
            raise ValueError("feature %r: expected (kind, z0, z1) or (kind, z0, z1, c)" % (name,))
        kind = spec[0]
        if not isinstance(kind, str) or kind not in FEATURE_KINDS:
            raise ValueError("feature %r: unknown kind %r (one of %s)" % (name, kind, ", ".join(FEATURE_KINDS)))
        if len(spec) == 4 and kind not in FEATURE_OPTIONAL:
            raise ValueError("feature %r: kind %r takes no c" % (name, kind))
        if len(spec) == 3 and kind == "above":
            raise ValueError("feature %r: kind 'above' needs c, the velocity to exceed" % (name,))
        vals = list(spec[1:]) + ([0.0] if len(spec) == 3 else [])
        for i, (what, v) in enumerate(zip(("z0", "z1", "c"), vals)):
            try:
                v = np.asarray(v, np.float64)
            except (TypeError, ValueError):
                raise ValueError("feature %r: %s must be a number or one number per site" % (name, what))
            if v.ndim > 1 or (v.ndim == 1 and v.shape[0] != S):
                raise ValueError("feature %r: %s must be one number or one per site (%d sites), not shape %r" % (name, what, S, v.shape))
            par[:, f, i] = v
        for s in range(S):
            z0, z1, c = par[s, f]
            at = "feature %r, site %d" % (name, s)
            if not (np.isfinite(z0) and np.isfinite(z1) and np.isfinite(c)):
                raise ValueError("%s: z0, z1 and c must be finite" % at)
            if z0 < 0:
                raise ValueError("%s: z0 = %r lies below 0 km" % (at, z0))
            if not z1 > z0:
                raise ValueError("%s: the window needs z0 < z1, not [%r, %r]" % (at, z0, z1))
            if kind in ("drop", "jump") and c < 0:
                raise ValueError("%s: c = %r must not be negative (a %s is asked for by its size)" % (at, c, kind))
        kinds.append(FEATURE_KINDS.index(kind))
        labels += ["%s.%s" % (name, part) for part in FEATURE_PARTS[kind]] if kind in FEATURE_PARTS else [name]
    if len(labels) > E.SCALARS_MAXCOLS:
        raise ValueError("features: %d columns (feature %r is the first too many), a call takes at most %d (BH_SCALARS_MAXCOLS)"
                         % (len(labels), labels[E.SCALARS_MAXCOLS].split(".")[0], E.SCALARS_MAXCOLS))
    return np.array(kinds, np.int32), par, labels


def posterior_features(models, features, site=None, bins=50, quantiles=None, engine=None, nsites=None, classes=None):
    """The posterior of structural features of every site's layered models: a list of dicts (one dict when site is None).
    features: a dict name -> (kind, z0, z1[, c]); every number a scalar or a sequence of one value per site.  With the row's step
    model (layer j from the interface above it to the one below, the last to infinity) and the window [z0, z1] km, the kinds are
      vsmean   the thickness-weighted mean vs of the window            vstime  its time-averaged vs (z1 - z0) / tts (Vs30-style)
      tts      the vertical S travel time through the window (s)       nifaces the number of interfaces inside the window
      vsmin, vsmax  the slowest / fastest layer of the window: value and the depth where it starts inside the window
      drop, jump    the strongest velocity decrease / increase across an interface inside the window, where it exceeds c (>= 0,
                    default 0): depth and jump; a row without one has no value
      above    the first interface inside the window below which vs exceeds c (sediment thickness with c a basement velocity; the
               Moho rule with the Moho's parameters): depth
    (the exact rules: include/bh_engine_posterior_features.h).  The dict holds rows, invalid_rows and dropped as posterior_moho's,
    and per feature name a statistics dict for a kind of one column -- count, nan, median, mean, std, min, max, constant, hist =
    (counts, edges), mode, and quantiles [R] where asked, as posterior_scalars' (edges: numpy.histogram_bin_edges(data, bins);
    nifaces arange(min, max + 2) - 0.5) -- and for a kind of two {"depth": statistics, "value" | "jump": statistics, "hist2d":
    (counts [bins, bins], xedges of the value or jump, yedges of the depth), "mode": (value or jump, depth), the centres of the first
    largest cell}.  drop, jump and above add probability = count / rows: the posterior probability that the station has such a
    feature (NaN for a site without rows).
    classes: the dict posterior_classes returned for the same rows: the result is then per site a dict class name -> the dict
    described here, of the rows of that class alone (posterior_classes says how rows in no class are accounted for)."""
    if classes is not None:
        return _by_class(posterior_features, classes, models, site, dict(features=features, bins=bins, quantiles=quantiles, engine=engine,
                                                                         nsites=nsites))
    qs = check_quantiles(quantiles)
    ld = _Loaded(models, site, engine, nsites, scalars=True)
    try:
        S = ld.S
        kinds, par, labels = check_features(features, S)
        ld.features(kinds, par)
        W = E.SCALARS_FEATURES
        st = ld.scalar_stats(W)
        qv = set_quantiles(ld, W, st["count"], qs) if qs is not None else None
        Q = len(labels)
        colkind = [FEATURE_KINDS[k] for k in kinds for _ in range(FEATURE_COLS[FEATURE_KINDS[k]])]
        edges = [[scalar_edges(st["min"][s, q], st["max"][s, q], np.float64, bins, colkind[q] == "nifaces")
                  if st["count"][s, q] else scalar_edges(None, None, np.float64, bins) for s in range(S)] for q in range(Q)]
        hists = [ld.scalar_hist(W, q, edges[q]) for q in range(Q)]
        e2, h2 = {}, {}
        q = 0
        for k in kinds:
            kind = FEATURE_KINDS[k]
            if kind in FEATURE_PARTS:
                qx, qy = (q, q + 1) if FEATURE_PARTS[kind][0] != "depth" else (q + 1, q)     # x: value or jump, y: depth
                both = [bool(st["count"][s, qx]) and bool(st["count"][s, qy]) for s in range(S)]
                e2[q] = [[moho_edges(st["min"][s, c], st["max"][s, c], bins) if both[s] else moho_edges(None, None, bins)
                          for s in range(S)] for c in (qx, qy)]
                h2[q] = ld.scalar_hist2d(W, qx, qy, e2[q][0], e2[q][1])
            q += FEATURE_COLS[kind]
    finally:
        ld.close()

    def stats(s, q):
        d = _stat_dict(st, s, q)
        n = int(st["count"][s, q])
        e = edges[q][s]
        cnt = hists[q][s].astype(np.int64)
        d.update(count=n, nan=int(st["nan"][s, q]), constant=bool(n and st["min"][s, q] == st["max"][s, q]), hist=(cnt, e),
                 mode=((e[:-1] + e[1:]) / 2.)[np.argmax(cnt)] if n else np.nan)
        if qs is not None:
            d["quantiles"] = qv[s, q].copy()
        return d

    out = []
    for s in range(S):
        rows = int(ld.rows[s])
        r = dict(rows=rows, invalid_rows=int(ld.invalid[s]), dropped=ld.dropped)
        q = 0
        for name, k in zip(features, kinds):
            kind = FEATURE_KINDS[k]
            if kind in FEATURE_PARTS:
                d = {part: stats(s, q + i) for i, part in enumerate(FEATURE_PARTS[kind])}
                counts, am = h2[q]
                xe, ye = e2[q][0][s], e2[q][1][s]
                d["hist2d"] = (counts[s].astype(np.int64), xe, ye)
                if counts[s].any():
                    xi, yi = divmod(int(am[s]), ye.size - 1)
                    d["mode"] = (((xe[:-1] + xe[1:]) / 2.)[xi], ((ye[:-1] + ye[1:]) / 2.)[yi])
                else:
                    d["mode"] = (np.nan, np.nan)
                n = d["depth"]["count"]
            else:
                d = stats(s, q)
                n = d["count"]
            if kind in FEATURE_OPTIONAL:
                d["probability"] = n / rows if rows else np.nan
            r[name] = d
            q += FEATURE_COLS[kind]
        out.append(r)
    return out[0] if site is None else out


# ---- conditional posteriors: the rows of a site split into classes (include/bh_engine_posterior_classes.h) ---------------------

CLASS_OPS = ("in", "has", "lacks")   # BH_CLASS_*, in order


def check_classes(classes, S, labels):
    """The user's rule as the arrays of bh_posterior_classes over S sites: (names [K], term_class, term_set, term_col, term_op
    int32 [T], lo, hi float64 [S, T]).  classes: an ordered dict class name -> list of terms, the first class whose terms all hold
    taking the row; a class with an empty list takes every row that is left.  A term is (label, lo, hi) -- the row has a value v
    in the column and lo <= v < hi; lo and hi one number or one per site, -inf and inf allowed --, (label, "has") -- the row has a
    value -- or (label, "lacks") -- it has none (NaN).  labels: a dict label -> (set, column), the columns the call has formed.
    Pure host code; every refused input is a ValueError that names the class (and the site, where one site's value is at fault)."""
    if not isinstance(classes, dict) or not classes:
        raise ValueError("classes must be a dict name -> list of terms with at least one entry")
    if len(classes) > E.CLASSES_MAX:
        raise ValueError("classes: %d classes (class %r is the first too many), a call takes at most %d (BH_CLASSES_MAX)"
                         % (len(classes), list(classes)[E.CLASSES_MAX], E.CLASSES_MAX))
    S = int(S)
    names, tc, ts, tq, to, los, his = [], [], [], [], [], [], []
    for k, (name, terms) in enumerate(classes.items()):
        if not isinstance(name, str) or not name:
            raise ValueError("class %r: the name must be a non-empty string" % (name,))
        if isinstance(terms, (str, bytes, dict)) or not hasattr(terms, "__len__"):
            raise ValueError("class %r: expected a list of terms (label, lo, hi), (label, 'has') or (label, 'lacks')" % (name,))
        for term in terms:
            if isinstance(term, (str, bytes)) or not hasattr(term, "__len__") or len(term) not in (2, 3):
                raise ValueError("class %r: a term is (label, lo, hi), (label, 'has') or (label, 'lacks'), not %r" % (name, term))
            label = term[0]
            if not isinstance(label, str) or label not in labels:
                raise ValueError("class %r: %r is no column of this call (%s)" % (name, label, ", ".join(labels) or "none formed"))
            if len(tc) == E.CLASS_MAXTERMS:
                raise ValueError("class %r: its term on %r is the first beyond the %d terms a call takes (BH_CLASS_MAXTERMS)"
                                 % (name, label, E.CLASS_MAXTERMS))
            lo, hi = np.full(S, -np.inf), np.full(S, np.inf)
            if len(term) == 2:
                if not isinstance(term[1], str) or term[1] not in ("has", "lacks"):
                    raise ValueError("class %r, column %r: a term of two is (label, 'has') or (label, 'lacks'), not %r"
                                     % (name, label, term[1]))
                op = CLASS_OPS.index(term[1])
            else:
                op = E.CLASS_IN
                for what, dst, v in (("lo", lo, term[1]), ("hi", hi, term[2])):
                    try:
                        v = np.asarray(v, np.float64)
                    except (TypeError, ValueError):
                        raise ValueError("class %r, column %r: %s must be a number or one number per site" % (name, label, what))
                    if v.ndim > 1 or (v.ndim == 1 and v.shape[0] != S):
                        raise ValueError("class %r, column %r: %s must be one number or one per site (%d sites), not shape %r"
                                         % (name, label, what, S, v.shape))
                    dst[:] = v
                for s in range(S):
                    at = "class %r, column %r, site %d" % (name, label, s)
                    if np.isnan(lo[s]) or np.isnan(hi[s]):
                        raise ValueError("%s: a bound is NaN" % at)
                    if lo[s] > hi[s]:
                        raise ValueError("%s: lo = %r lies above hi = %r" % (at, float(lo[s]), float(hi[s])))
            tc.append(k)
            ts.append(labels[label][0])
            tq.append(labels[label][1])
            to.append(op)
            los.append(lo)
            his.append(hi)
        names.append(name)
    if len(set(names)) != len(names):
        raise ValueError("classes: a class name occurs twice")
    T = len(tc)
    lo = np.ascontiguousarray(np.array(los, np.float64).reshape(T, S).T)
    hi = np.ascontiguousarray(np.array(his, np.float64).reshape(T, S).T)
    return names, np.array(tc, np.int32), np.array(ts, np.int32), np.array(tq, np.int32), np.array(to, np.int32), lo, hi


def _is_tensor(v):
    try:
        import torch
    except ImportError:
        return False
    return isinstance(v, torch.Tensor)


def posterior_classes(models, classes, site=None, features=None, moho=None, mohovs=MOHOVS, columns=None, nlayers=False, engine=None,
                      nsites=None, return_columns=False):
    """Split every site's rows into classes by a rule over their scalar columns, on the device: what a bimodal posterior needs
    before it is summarised -- a mean over two Moho candidates describes a model no chain sampled.
    classes: an ordered dict class name -> list of terms (check_classes): (label, lo, hi), (label, "has"), (label, "lacks"); the
    first class whose terms all hold takes the row.  The labels are those of the sources given, any of them at once:
      features: as posterior_features' -- the labels check_features returns (name, name.depth, name.jump, name.value);
      moho = (lo, hi) or one pair per site, with mohovs: as posterior_moho's -- "moho", "vslast", "vscrust", "vsjump";
      columns: as posterior_scalars', one value row per model row -- name, or name[0] .. name[k-1] for a [N, k] column; nlayers:
        "nlayers".
    Returns a dict: names [K]; cls int32 [N], every input row's class in the input's order, -1 for a row in no class and for a
    row the load leaves out (a NaN row, a malformed row, a device row whose site is out of range) -- a numpy array for numpy rows, a
    device tensor for a device tensor; counts [S, K], unclassified [S], rows [S] (counts.sum(1) + unclassified == rows);
    probability [S, K] = counts / rows (NaN for a site without rows); nclasses = K; site int32 [N] = site * K + cls, -1 where
    either is negative, and nsites = S * K: every class of every site as a site of its own; with return_columns, columns: label
    -> float64 [N], every source column by input row (NaN where the load left the row out).
    The dict is what classes= of posterior_models, posterior_hist2d, posterior_moho, posterior_scalars, posterior_features and
    posterior_covariance takes, with the same rows (and the same site, or None): the call then runs on the S * K virtual sites,
    per-site arguments (moho, mohovs, the numbers of features) repeated for every class of the site and per-row arguments (misfits,
    columns) passed through, and returns per site a dict class name -> the function's usual dict (a list over sites when site is
    given).  The numbers of a class are those of the function called on the rows of that class alone, bit for bit.  Rows in no
    class: numpy rows are removed before the load (rows, invalid_rows and dropped are those of the class's own rows); device
    tensors stay where they are, these rows get site -1 and are counted in `dropped`, the total of the call.
    cls and counts are predicates on float64 columns that are exact functions of the rows: the same bits alone or among other
    sites, in any row order, from host or device memory, on every repeat."""
    ld = _Loaded(models, site, engine, nsites, scalars=True)
    try:
        S = ld.S
        labels, formed = {}, []

        def take(new, which):
            for i, lb in enumerate(new):
                if lb in labels:
                    raise ValueError("label %r names two columns of this call: rename the feature or the column" % (lb,))
                labels[lb] = (which, i)
            formed.append((which, list(new)))

        if features is not None:
            kinds, par, flabels = check_features(features, S)
            take(flabels, E.SCALARS_FEATURES)
        if moho is not None:
            rng = _per_site(moho, S, 2, "moho")
            mv = _per_site(mohovs, S, 0, "mohovs")
            take(MOHO_COLUMNS, E.SCALARS_MOHO)
        values, layout = _stack_columns(columns, ld.N) if columns is not None else (None, [])
        if values is not None or nlayers:
            take([name if idx is None else "%s[%d]" % (name, idx) for name, idx, _ in layout] + (["nlayers"] if nlayers else []),
                 E.SCALARS_USER)
        names, tc, ts, tq, to, lo, hi = check_classes(classes, S, labels)
        if features is not None:
            ld.features(kinds, par)
        if moho is not None:
            ld.moho(rng[:, 0], rng[:, 1], mv)
        if values is not None or nlayers:
            ld.attach(values, nlayers)
        K = len(names)
        dev = models.device if _is_tensor(models) else None
        cls, cnt = ld.classes(K, tc, ts, tq, to, lo, hi, device=dev)
        cols = None
        if return_columns:
            cols = {}
            for which, lbs in formed:
                tab = ld.export(which, device=dev)
                for i, lb in enumerate(lbs):
                    cols[lb] = tab[:, i]
    finally:
        ld.close()
    rows = ld.rows.copy()
    counts = cnt[:, :K].copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        prob = np.where(rows[:, None] > 0, counts / rows[:, None].astype(np.float64), np.nan)
    if dev is None:
        st = np.zeros(ld.N, np.int32) if site is None else np.asarray(site).astype(np.int32)
        vsite = np.where((st >= 0) & (cls >= 0), st * np.int32(K) + cls, np.int32(-1)).astype(np.int32)
    else:
        import torch
        st = torch.zeros_like(cls) if site is None else torch.as_tensor(site, device=dev).to(torch.int32)
        vsite = torch.where((st >= 0) & (cls >= 0), st * K + cls, torch.full_like(cls, -1)).to(torch.int32)
    out = dict(names=names, cls=cls, counts=counts, unclassified=cnt[:, K].copy(), rows=rows, probability=prob, nclasses=K, site=vsite,
               nsites=S * K)
    if cols is not None:
        out["columns"] = cols
    return out


def _repeat_features(features, S, K):
    """the features dict with every number given per virtual site: each site's value K times"""
    check_features(features, S)
    return {name: (spec[0],) + tuple(np.repeat(np.broadcast_to(np.asarray(v, np.float64), (S,)), K) for v in spec[1:])
            for name, spec in features.items()}


def _rows_of(v, keep):
    if v is None:
        return None
    if _is_tensor(v):
        import torch
        return v[torch.from_numpy(keep).to(v.device)]
    return np.asarray(v)[keep]


def _by_class(fn, classes, models, site, kw):
    """fn(models, ...) over the virtual sites of a posterior_classes dict: per site a dict class name -> fn's dict"""
    if not isinstance(classes, dict) or not all(k in classes for k in ("names", "site", "nclasses", "nsites")):
        raise ValueError("classes must be the dict posterior_classes returned for these rows")
    names, K = list(classes["names"]), int(classes["nclasses"])
    S = int(classes["nsites"]) // K
    vsite = classes["site"]
    if len(models.shape) != 2 or int(vsite.shape[0]) != int(models.shape[0]):
        raise ValueError("classes holds %d rows, models %d: the dict must stem from the same rows" % (int(vsite.shape[0]), int(models.shape[0])))
    if site is None and S != 1:
        raise ValueError("classes was formed over %d sites: give the same site index" % S)
    if kw.get("nsites") is not None and int(kw["nsites"]) != S:
        raise ValueError("classes was formed over %d sites, nsites is %d" % (S, int(kw["nsites"])))
    kw = dict(kw)
    if kw.get("moho") is not None:
        kw["moho"] = np.repeat(_per_site(kw["moho"], S, 2, "moho"), K, axis=0)
        kw["mohovs"] = np.repeat(_per_site(kw["mohovs"], S, 0, "mohovs"), K)
    if kw.get("features") is not None:
        kw["features"] = _repeat_features(kw["features"], S, K)
    if _is_tensor(models):
        import torch
        vsite = torch.as_tensor(vsite, device=models.device)
    else:
        if _is_tensor(vsite):
            vsite = vsite.detach().cpu().numpy()
        models = np.asarray(models)
        keep = np.asarray(vsite) >= 0   # the host load refuses a site out of range: the rows in no class go before it
        models, vsite = models[keep], np.asarray(vsite)[keep]
        if kw.get("misfits") is not None:
            kw["misfits"] = _rows_of(kw["misfits"], keep)
        if kw.get("columns") is not None:
            kw["columns"] = {name: _rows_of(v, keep) for name, v in kw["columns"].items()}
    kw["nsites"] = S * K
    res = fn(models, site=vsite, **kw)
    out = [{names[k]: res[s * K + k] for k in range(K)} for s in range(S)]
    return out if site is not None else out[0]
