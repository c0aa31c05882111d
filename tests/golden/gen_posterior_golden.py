#!/usr/bin/env python3
"""Generate tests/golden/posterior_golden.npz from the REAL reference's posterior helpers.

Runs only where the reference is present: it loads the reference's own src/Models.py, unmodified.  For seeded model sets
in three dtypes -- float32 rows (chain files c???_p2models.npy), float64 rows holding float32 values (c_models.npy) and
general float64 rows -- it stores the reference's own
  * ModelMatrix.get_interpmodels (the interpolated vs of every row) on the default 0.5 km grid,
  * the statistics of ModelMatrix.get_singlemodels (src/Models.py:176-207), the mode's histogram2d included, and
    Model.get_stepmodel of the best-misfit row,
  * the 2-D plot's histograms (_plot_bestmodels_hist, src/Plotting.py:460-495) for a 1 km dep_int.
Nothing of the reference is copied: the file holds data only.

    python tests/golden/gen_posterior_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True


def model_sets(rs, jitter=0.0):
    """Rows with the cases the rule must hold on: two nuclei in the top 10 m, interfaces on grid depths, zero-thickness
    layers (the first at depth 0), one-layer rows, NaN-only rows.  jitter: relative noise on vs and z (general float64
    values; z stays sorted)."""
    ML, N = 21, 1800
    rows = np.full((N, 2 * ML), np.nan)
    for i in range(N):
        kind = i % 6
        n = rs.randint(1, ML + 1)
        z = np.sort(rs.uniform(0, 60, n))
        if kind == 1 and n >= 3:
            z[:2] = np.sort(rs.uniform(0, 0.01, 2))                       # two nuclei in the top 10 m
        elif kind == 2 and n >= 2:
            z = np.sort(rs.randint(0, 120, n).astype(float)) / 2.        # zd on the 0.25 km lattice: many on the grid
        elif kind == 3 and n >= 4:
            z[:2] = 0.0                                                   # first interface at depth 0
            z[n // 2 + 1] = z[n // 2] = z[n // 2 - 1]                     # zero-thickness layer inside
            z = np.sort(z)
        elif kind == 4:
            n, z = 1, rs.uniform(0, 50, 1)
        vs = rs.uniform(2.0, 4.8, n)
        if jitter:
            vs = vs * (1 + rs.uniform(-jitter, jitter, n))
            z = np.sort(z * (1 + rs.uniform(-jitter, jitter, n)))
        rows[i, :n], rows[i, n:2 * n] = vs, z
    rows[::97] = np.nan                                                   # NaN-only rows are dropped
    return rows


def main():
    import importlib.util
    ref = os.environ.get("BH_REFERENCE", "/root/reference")
    spec = importlib.util.spec_from_file_location("ref_models", os.path.join(ref, "src", "Models.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    rs = np.random.RandomState(20261015)
    base = model_sets(rs)
    sets = {"f32": base.astype(np.float32),
            "f64of32": base.astype(np.float32).astype(np.float64),
            "f64": model_sets(np.random.RandomState(20261016), jitter=1e-9)}
    out = {}
    dep = np.linspace(0, 100, 201)
    out["dep_int"] = dep
    for key, models in sets.items():
        misfits = rs.uniform(0.1, 2.0, len(models))
        misfits[len(models) // 3] = 0.01
        vsi, _ = M.ModelMatrix.get_interpmodels(models, dep)
        out[key + "_models"] = models
        out[key + "_misfits"] = misfits
        out[key + "_vsi"] = vsi
        # get_singlemodels (src/Models.py:183-213), statement by statement: its mode line
        # `bins, vs_bin, dep_bin = np.array(data).T` (src/Models.py:205) fails on numpy >= 1.24 (ragged tuple), so the
        # same histogram2d result is taken apart directly.
        out[key + "_mean"] = np.mean(vsi, axis=0)
        out[key + "_median"] = np.median(vsi, axis=0)
        out[key + "_min"], out[key + "_max"] = np.min(vsi, axis=0), np.max(vsi, axis=0)
        out[key + "_std"] = np.std(vsi, axis=0)
        flat = vsi.flatten()
        vsbins = int((flat.max() - flat.min()) / 0.025)
        bins, vs_bin, dep_bin = np.histogram2d(flat, np.repeat([dep], len(vsi), axis=0).flatten(), bins=(vsbins, dep))
        out[key + "_modecounts"] = bins.astype(np.int64)
        out[key + "_mode"] = ((vs_bin[:-1] + vs_bin[1:]) / 2.)[np.argmax(bins.T, axis=1)]
        out[key + "_dep_center"] = (dep_bin[:-1] + dep_bin[1:]) / 2.
        _, vsb, depb = M.Model.get_stepmodel(models[np.argmin(misfits)])
        out[key + "_best_vs"], out[key + "_best_dep"] = vsb, depb
        # _plot_bestmodels_hist with dep_int = np.arange(0, 61, 1.) (src/Plotting.py:460-495, the inline numpy calls)
        di = np.arange(0, 61, 1.)
        maxdepth = int(np.ceil(di.max()))
        interp = di[1] - di[0]
        samples = np.arange(di[0], di[-1] + interp / 2., interp / 2.)
        depbins = np.arange(0, maxdepth + 2 * interp, interp)
        m2 = M.ModelMatrix._replace_zvnoi_h(models)
        m2 = [m[~np.isnan(m)] for m in m2]
        yinterf = np.concatenate([np.cumsum(m[int(m.size / 2):-1]) for m in m2])
        vsi2, deps2 = M.ModelMatrix.get_interpmodels(models, samples)
        f2 = vsi2.flatten()

        def vs_round(vs):  # src/Plotting.py:29-32
            vs_floor = np.floor(vs)
            return np.round((vs - vs_floor) * 40) / 40 + vs_floor
        vsedges = np.arange(vs_round(f2.min()) - 2 * 0.025, vs_round(f2.max()) + 3 * 0.025, 0.025)
        data2d, xe, ye = np.histogram2d(f2, deps2.flatten(), bins=(vsedges, depbins))
        out[key + "_h2_samples"], out[key + "_h2_depbins"], out[key + "_h2_vsedges"] = samples, depbins, xe
        out[key + "_h2_counts"] = data2d.astype(np.int64)
        out[key + "_h2_interfaces"] = np.histogram(yinterf, bins=depbins)[0].astype(np.int64)
    np.savez_compressed(os.path.join(HERE, "posterior_golden.npz"), **out)
    print("wrote", os.path.join(HERE, "posterior_golden.npz"), os.path.getsize(os.path.join(HERE, "posterior_golden.npz")))


if __name__ == "__main__":
    main()
