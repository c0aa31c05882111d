#!/usr/bin/env python3
"""Generate tests/golden/datafit_golden.npz from the REAL reference (arrays only).

Runs only where the reference is present (imported the way gen_golden.py imports it, unmodified).  For seeded model rows in
three dtypes -- float32 rows with float32 vpvs, float64 rows holding float32 values and general float64 rows -- it stores vp, vs
and h of the reference's own Model.get_vp_vs_h and rho of plot_bestdatafits' expression `vp * 0.32 + 0.77`, without and with
a mantle rule, in the dtypes the reference returns them in.  (Model.get_vp has a line with `np.int`, which current numpy
lacks: gen_golden.import_reference serves the name, and the Models module's `np` goes through a forwarding stand-in that
has it too.  The method is not copied.)

It also stores the rows the reference's best-fit selection picks: PlotFromStorage.plot_bestmodels -- whose per-chain
argmin and best-of-all loop are, line for line, those of plot_bestdatafits, and which needs no forward plugin -- runs under
the Agg backend over seeded chain files with ties and an outlier chain, and the stand-in for the Plotting module's `np`
writes down what np.argmin returned for every chain file it was asked about.

    python tests/golden/gen_datafit_golden.py
"""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

ML = 21
MANTLE = (4.2, 1.8)


def layer_rows(rs, jitter=0.0):
    """rows of 1 to 21 layers: every count twice at random, then the cases the mantle rule must hold on"""
    rows, vpvs = [], []

    def add(vs, z, k):
        r = np.full(2 * ML, np.nan)
        n = len(vs)
        r[:n], r[n:2 * n] = vs, z
        rows.append(r)
        vpvs.append(k)

    for n in list(range(1, ML + 1)) * 2:
        vs = rs.uniform(2.0, 4.8, n)
        z = np.sort(rs.uniform(0, 80, n))
        if jitter:
            vs = vs * (1 + rs.uniform(-jitter, jitter, n))
        add(vs, z, rs.uniform(1.5, 2.0))
    add([3.1], [12.0], 1.73)                                         # one layer, crust
    add([4.6], [12.0], 1.73)                                         # one layer, mantle
    add([3.0, 3.5, MANTLE[0], 4.5], [2.0, 10.0, 30.0, 50.0], 1.7)    # a vs exactly mantle_vs
    add([4.4, 3.0, 3.2], [1.0, 5.0, 9.0], 1.8)                       # the mantle reached in the first layer: all below follow
    add([2.5, 3.0, 3.5, 4.0], [1.0, 5.0, 9.0, 30.0], 1.9)            # never
    add([3.0, 4.3, 3.1, 4.5], [3.0, 3.0, 8.0, 8.0], 1.65)            # a slow layer below the first mantle layer; equal depths
    return np.array(rows), np.array(vpvs)


def main():
    import gen_golden
    gen_golden.import_reference()
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    import BayHunter.Models as M
    import BayHunter.Plotting as P
    from gen_moho_golden import ForwardNumpy

    class WithInt(ForwardNumpy):
        int = int

    M.np = WithInt(np, [])
    base, kbase = layer_rows(np.random.RandomState(20261101))
    gen, kgen = layer_rows(np.random.RandomState(20261102), jitter=1e-9)
    sets = {"f32": (base.astype(np.float32), kbase.astype(np.float32)),
            "f64of32": (base.astype(np.float32).astype(np.float64), kbase.astype(np.float32).astype(np.float64)),
            "f64": (gen, kgen)}
    out = dict(mantle=np.array(MANTLE))
    for key, (rows, vpvs) in sets.items():
        out[key + "_rows"], out[key + "_vpvs"] = rows, vpvs
        for tag, mantle in (("plain", None), ("mantle", list(MANTLE))):
            vp_all = np.zeros((len(rows), ML), rows.dtype)
            vs_all = np.zeros((len(rows), ML), rows.dtype)
            rho_all = np.zeros((len(rows), ML), rows.dtype)
            h_all = np.zeros((len(rows), ML), np.float64)
            nl = np.zeros(len(rows), np.int32)
            for i, (row, k) in enumerate(zip(rows, vpvs)):
                vp, vs, h = M.Model.get_vp_vs_h(row, k, mantle)
                rho = vp * 0.32 + 0.77
                n = len(vs)
                assert vp.dtype == vs.dtype == rho.dtype == rows.dtype and h.dtype == np.float64 and len(h) == n, (key, i)
                nl[i] = n
                vp_all[i, :n], vs_all[i, :n], rho_all[i, :n], h_all[i, :n] = vp, vs, rho, h
            for name, a in (("vp", vp_all), ("vs", vs_all), ("rho", rho_all), ("h", h_all), ("nlay", nl)):
                out["%s_%s_%s" % (key, tag, name)] = a
    M.np = np

    # the best-fit selection: chain files with ties, chain 2 an outlier
    log = []

    class LogArgmin(ForwardNumpy):
        def argmin(self, a, *args, **kw):
            i = self._real.argmin(a, *args, **kw)
            self._log.append((self._real.array(a, dtype=self._real.float64), int(i)))
            return i

    P.np = LogArgmin(np, log)
    rs = np.random.RandomState(20261103)
    tmp = tempfile.mkdtemp(prefix="bhfit_")
    try:
        nch, files, chain_mis = 5, [], []
        for c in range(nch):
            n = 40 + 7 * c
            mis = np.round(rs.uniform(0.1, 0.5, (n, 3)), 2).astype(np.float32).astype(np.float64)   # (two decimals: ties)
            lo = mis[:, -1].min()
            mis[rs.randint(0, n, 3), -1] = lo                                                        # ... and the least repeated
            if c == 3:
                mis[:, -1] = 0.25                                                                    # a constant chain
            models = np.full((n, 8), np.nan)
            models[:, :2] = rs.uniform(2.5, 4.5, (n, 2))
            models[:, 2:4] = np.sort(rs.uniform(0, 40, (n, 2)), axis=1)
            f = os.path.join(tmp, "c%03d_p2models.npy" % c)
            np.save(f, models)
            np.save(f.replace("models", "vpvs"), rs.uniform(1.6, 1.9, n))
            np.save(f.replace("models", "misfits"), mis)
            files.append(f)
            chain_mis.append(mis[:, -1])
        pl = object.__new__(P.PlotFromStorage)
        pl.datapath, pl.priors, pl.mantle = tmp, {"z": (0, 60), "vs": (2, 5)}, None
        pl.modfiles = [[], files]
        pl.outliers = np.array([2.0])
        fig = pl.plot_bestmodels()
        assert fig is not None, "the reference's method did not run through"
        plt.close("all")
        kept = [c for c in range(nch) if c != 2]
        assert len(log) == 3 * len(kept)                       # (three np.argmin per chain file, the outlier's skipped)
        picks = np.full(nch, -1, np.int64)
        for j, c in enumerate(kept):
            a, i = log[3 * j]
            assert np.array_equal(a, chain_mis[c])
            picks[c] = i
        out["best_nchains"] = nch
        out["best_outlier"] = 2
        out["best_misfits"] = np.concatenate(chain_mis)
        out["best_chain"] = np.concatenate([np.full(len(m), c, np.int32) for c, m in enumerate(chain_mis)])
        out["best_picks"] = picks                              # the row inside every chain's own file
    finally:
        P.np = np
        shutil.rmtree(tmp, ignore_errors=True)
    path = os.path.join(HERE, "datafit_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "picks", picks)


if __name__ == "__main__":
    main()
