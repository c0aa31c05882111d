#!/usr/bin/env python3
"""Generate tests/golden/moho_golden.npz from the REAL reference's posterior plots.

Runs only where the reference is present (imported the way gen_golden.py imports it, unmodified).  For seeded model sets in
three dtypes -- float32 rows, float64 rows holding float32 values (c_models.npy) and general float64 rows -- it runs the
reference's own PlotFromStorage.plot_moho_crustvel_tradeoff under the Agg backend on c_models.npy / c_vpvs.npy in a temporary
folder, on an instance made with datapath, priors and mantle = None (the mantle rule only touches vp, which the result does
not use, and its np.int line breaks on current numpy), and stores
  * the four per-row arrays (moho, vslast, vscrust, vsjump of the rows with a Moho) that the method hands to np.median --
    captured by giving the imported Plotting module a forwarding stand-in for its `np` name,
  * the bar heights of the four 1-D histograms, the QuadMesh counts of the three 2-D histograms, and the medians.
For seeded float64-of-float32 c_likes / c_misfits / c_vpvs / c_noise / c_models it runs plot_posterior_likes / _misfits /
_nlayers / _vpvs / _noise / _others and stores the bar heights and medians.  It also stores the seconds the reference's loop
over the posterior models takes per 10 000 rows on this CPU.  Nothing of the reference is copied: the file holds data only.

    python tests/golden/gen_moho_golden.py
"""
import os
import shutil
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

LO, HI, MOHOVS = 10.0, 45.0, 4.2   # the Moho range and mantle vs of every set
ML, N = 21, 1800
CRUST = (3, 8, 12, 16, 18)         # crustal layers above the Moho: < 8, 8, 9-15, 16, > 16


def moho_model_sets(rs, jitter=0.0):
    """Rows with the cases the rule must hold on (kind = i % 12).  jitter: relative noise on vs and z of the kinds without an
    exact coincidence (general float64 values; z stays sorted)."""
    rows = np.full((N, 2 * ML), np.nan)
    for i in range(N):
        kind = i % 12
        jit = jitter
        if kind in (0, 9):                                   # anything: vs and z at random
            n = rs.randint(1, ML + 1)
            z, vs = np.sort(rs.uniform(0, 60, n)), rs.uniform(2.0, 4.8, n)
        elif kind in (1, 2, 3, 10, 11):                      # a crust of nc layers over a mantle of 2
            nc = CRUST[(i // 12) % len(CRUST)]
            n = nc + 2
            z = np.concatenate((np.sort(rs.uniform(0, 28, nc)), np.sort(rs.uniform(30, 44, 2))))
            vs = np.concatenate((np.sort(rs.uniform(2.0, 4.1, nc)), rs.uniform(4.25, 4.8, 2)))
        elif kind == 4:                                      # an interface exactly at LO (strict: not the Moho), a Moho below
            jit = 0.0
            z = np.array([2.0, 8.0, 12.0, 30.0, 36.0])       # zd = 5, 10, 21, 33
            vs = np.array([3.0, 3.5, 4.5, 3.9, 4.6])
            if (i // 12) % 2:
                z, vs = z[:3], vs[:3]                        # ... or none: the interface at LO is the only candidate
            n = len(z)
        elif kind == 5:                                      # an interface exactly at HI, vs above mohovs below it
            jit = 0.0
            z, vs = np.array([1.0, 5.0, 40.0, 50.0]), np.array([3.0, 3.4, 3.8, 4.6])   # zd = 3, 22.5, 45
            n = 4
        elif kind == 6:                                      # a vs exactly mohovs below the first candidate (strict)
            jit = 0.0
            z, vs = np.array([5.0, 25.0, 35.0, 41.0]), np.array([3.2, 3.7, MOHOVS, 4.4 + 0.01 * (i % 7)])   # zd = 15, 30, 38
            n = 4
        elif kind == 7:                                      # vs_1 above mohovs: no interface above it
            n = rs.randint(2, 8)
            z, vs = np.sort(rs.uniform(0, 50, n)), np.sort(rs.uniform(4.3, 4.8, n))
            if (i // 12) % 2:
                vs[1:] = rs.uniform(2.5, 4.0, n - 1)         # ... and slow below
        else:                                                # (8) one-layer rows; the only candidate fails the vs test
            if (i // 12) % 2:
                n, z, vs = 1, rs.uniform(0, 50, 1), rs.uniform(2.0, 4.8, 1)
            else:
                n = 4
                z = np.array([1.0, 3.0, rs.uniform(25, 40), rs.uniform(80, 90)])       # zd: 2, one inside, one below HI
                vs = np.array([4.5, 3.0, 3.6, 4.7])
        if jit:
            vs = vs * (1 + rs.uniform(-jit, jit, n))
            z = np.sort(z * (1 + rs.uniform(-jit, jit, n)))
        if kind == 3 and n >= 10:
            z[3:6] = z[3]                                    # zero-thickness layers inside the crust
        rows[i, :n], rows[i, n:2 * n] = vs, z
    rows[::97] = np.nan                                      # NaN-only rows are dropped
    return rows


def scalar_sets(rs, models):
    """float64-of-float32 c_likes / c_misfits / c_vpvs / c_noise of a run with two targets"""
    n = len(models)
    f = lambda a: a.astype(np.float32).astype(np.float64)
    likes = f(rs.normal(850., 12., n))
    misfits = f(np.abs(rs.normal(0.08, 0.02, (n, 3))))
    vpvs = f(rs.uniform(1.4, 2.1, n))
    noise = np.empty((n, 4))
    noise[:, 0] = 0.0                                        # constant correlations
    noise[:, 1] = rs.uniform(1e-3, 5e-2, n)
    noise[:, 2] = 0.98
    noise[:, 3] = rs.uniform(1e-2, 1e-1, n)
    return likes, misfits, vpvs, f(noise)


class ForwardNumpy(object):
    """The module `numpy` with np.median's arguments and results written down, and with the ragged np.array of the numpy the
    reference was written for (plot_posterior_nlayers / _others list the rows without their NaN)."""

    def __init__(self, real, log):
        self.__dict__["_real"], self.__dict__["_log"] = real, log

    def __getattr__(self, name):
        return getattr(self._real, name)

    def array(self, a, *args, **kw):
        try:
            return self._real.array(a, *args, **kw)
        except ValueError:                                   # rows of different lengths: the object array of numpy < 1.24
            return self._real.array(a, *args, dtype=object, **kw)

    def median(self, a, *args, **kw):
        m = self._real.median(a, *args, **kw)
        self._log.append((self._real.array(a, dtype=self._real.float64), float(m)))
        return m


def bars(ax, horizontal=False):
    return np.array([(p.get_width() if horizontal else p.get_height()) for p in ax.patches], dtype=np.float64)


def main():
    import gen_golden
    gen_golden.import_reference()
    import matplotlib.pyplot as plt
    P = sys.modules.get("BayHunter.Plotting")
    if P is None:
        import BayHunter.Plotting as P
    log = []
    P.np = ForwardNumpy(np, log)
    base = moho_model_sets(np.random.RandomState(20261018))
    sets = {"f32": base.astype(np.float32),
            "f64of32": base.astype(np.float32).astype(np.float64),
            "f64": moho_model_sets(np.random.RandomState(20261019), jitter=1e-9)}
    out = dict(lo=LO, hi=HI, mohovs=MOHOVS, bins=50)
    tmp = tempfile.mkdtemp(prefix="bhmoho_")
    try:
        def instance():
            pl = object.__new__(P.PlotFromStorage)
            pl.datapath, pl.priors, pl.mantle = tmp, {"z": (LO, HI)}, None
            pl.refs, pl.ntargets = ["rdispph", "prf", "joint"], 2
            return pl

        def run_moho(models):
            np.save(os.path.join(tmp, "c_models.npy"), models)
            np.save(os.path.join(tmp, "c_vpvs.npy"), np.full(len(models), 1.73))
            del log[:]
            t0 = time.perf_counter()
            fig = instance().plot_moho_crustvel_tradeoff(moho=None, mohovs=MOHOVS)
            dt = time.perf_counter() - t0
            assert fig is not None and len(log) == 4, "the reference's method did not run through"
            return fig, dt

        seconds = {}
        for key, models in sets.items():
            fig, seconds[key] = run_moho(models)
            ax = np.array(fig.axes).reshape(2, 4)
            (vslast, m1), (vscrust, m2), (vsjump, m3), (moho, m0) = log
            out[key + "_models"] = models
            out[key + "_values"] = np.stack((moho, vslast, vscrust, vsjump), axis=1)
            out[key + "_medians"] = np.array([m0, m1, m2, m3])
            share = len(moho) / float(np.sum(~np.isnan(models).all(1)))
            assert share >= 1. / 3., (key, share)
            out[key + "_share"] = share
            out[key + "_hist"] = np.stack([bars(ax[1][3], True)] + [bars(ax[0][n]) for n in range(3)]).astype(np.int64)
            h2 = []
            for n in range(3):
                arr = np.asarray(ax[1][n].collections[0].get_array()).reshape(50, 50)   # [ny, nx]: pcolormesh of counts.T
                h2.append(arr.T)
            out[key + "_hist2d"] = np.stack(h2).astype(np.int64)
            plt.close("all")
        # the loop's seconds per 10 000 rows: the slope between one and six copies of a set (the plotting is the same)
        big = np.tile(sets["f64of32"], (6, 1))
        _, t6 = run_moho(big)
        plt.close("all")
        _, t1 = run_moho(sets["f64of32"])
        plt.close("all")
        out["ref_loop_seconds_per_10000_rows"] = (t6 - t1) / (len(big) - len(sets["f64of32"])) * 1e4

        # the scalar posteriors
        models = sets["f64of32"]
        models = models[~np.isnan(models).all(1)]            # (a row of NaN only is no model: the runs write none)
        rs = np.random.RandomState(20261020)
        likes, misfits, vpvs, noise = scalar_sets(rs, models)
        for name, a in (("models", models), ("likes", likes), ("misfits", misfits), ("vpvs", vpvs), ("noise", noise)):
            np.save(os.path.join(tmp, "c_%s.npy" % name), a)
            out["sc_" + name] = a
        for meth in ("likes", "misfits", "nlayers", "vpvs", "noise", "others"):
            del log[:]
            fig = getattr(instance(), "plot_posterior_" + meth)()
            assert fig is not None, meth
            for i, ax in enumerate(fig.axes):
                out["sc_%s_%d_hist" % (meth, i)] = bars(ax).astype(np.int64)
                out["sc_%s_%d_median" % (meth, i)] = log[i][1]
            assert len(log) == len(fig.axes)
            plt.close("all")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    path = os.path.join(HERE, "moho_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), {k: round(float(out[k + "_share"]), 3) for k in sets},
          "ref loop s / 10000 rows: %.3f" % out["ref_loop_seconds_per_10000_rows"])


if __name__ == "__main__":
    main()
