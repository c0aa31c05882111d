"""A plain restatement of the feature series of the chains (include/bh_engine_chain_diag_features.h) and of the rule for rows that
lack a feature (bayhunter_amd/diagnostics.py: feature_convergence), on top of tests/features_ref.py: numpy and Python loops only,
nothing of the package.

value[t][k][q] is the column's value and +0.0 where the row lacks it, present[t][k][q] the indicator, missing[k][q] the count.  For
the kept series idx (ascending) of a site, with mean_c(a) the chain means handed in (x0 + S1 / T of the sums' tables):
    complete[q]    = no kept row lacks the column
    probability[q] = kept rows with a value / kept rows
    m[q]           = (sum_c mean_c(value)) / (sum_c mean_c(present)), both sums ascending from 0.0
    x              = value where complete, present * (value - m) otherwise (float64, the subtraction rounded before the product)
    sd(x)          = sqrt((sum_c P_{c,0} + T * sum_c (mean_c - g)^2) / (m T - 1)),  g = (sum_c mean_c) / m, sums ascending from 0.0
"""
import numpy as np

import features_ref as FR


def series_ref(models, kinds, par, site_of_series, sel=None):
    """(value float64 [T][K][Q], present float32 [T][K][Q], missing int64 [K][Q]) of models [T][C][2*ML]"""
    models = np.asarray(models)
    if sel is not None:
        models = np.take_along_axis(models, np.asarray(sel, np.int64)[:, :, None], 1)
    T, K = models.shape[:2]
    site = np.tile(np.asarray(site_of_series), T)
    tab = FR.features_ref(models.reshape(T * K, -1), kinds, par, site)            # [Q][T*K]
    tab = tab.T.reshape(T, K, -1)
    present = ~np.isnan(tab)
    value = np.where(present, tab, 0.0)
    return value, present.astype(np.float32), (~present).sum(axis=0).astype(np.int64)


def ascending(v):
    acc = np.zeros(np.shape(v)[1:])
    for row in v:
        acc = acc + row
    return acc


def missing_rule(value, present, missing, idx, mean_v, mean_p):
    """dict of complete, probability, m [Q] and x [T][m][Q] for the kept series idx, from the chain means mean_v, mean_p [K][Q]"""
    T = value.shape[0]
    complete = missing[idx].sum(axis=0) == 0
    n = len(idx) * T
    with np.errstate(all="ignore"):
        prob = (n - missing[idx].sum(axis=0)) / float(n)
        m = ascending(mean_v[idx]) / ascending(mean_p[idx])
    v, p = value[:, idx].astype(np.float64), present[:, idx].astype(np.float64)
    x = np.where(complete, v, p * (v - np.where(np.isnan(m), 0.0, m)))
    return dict(complete=complete, probability=prob, m=m, x=x)


def pooled_sd(tab, idx):
    """the pooled deviation [Q] over the chains idx from a table of sums (x0, s1, p, T)"""
    T, m = tab["T"], len(idx)
    mean = tab["x0"][idx] + tab["s1"][idx] / T
    g = ascending(mean) / m
    return np.sqrt((ascending(tab["p"][idx][:, :, 0]) + T * ascending((mean - g) * (mean - g))) / (m * T - 1))
