"""Every path of the posterior velocity-depth kernels (bayhunter_amd/csrc/posterior_kernel.hip: load and scatter, the column
passes, the histograms, the interface counts) against tests/posterior_ref.py, which tests/test_posterior_ref.py holds to the
reference's own outputs.  A site's reference is computed on the host from that site's rows alone.  Everything the kernels return
is a count, a selection or an integer sum, so every check is bit for bit; the one derived bound is the std's: 1 ulp of the exact
population std (an integer square root carried to 100 bits), from posterior._mean_std's q >= 2^60 truncated (2^-60 relative)
plus one correctly rounded division.

Rows come from `synth` (as tests/test_gpu_posterior.py::synth) and from its grid variant: nucleus depths on a 0.25 grid and vs on
a 1/32 grid, so that interfaces fall on multiples of 0.125 and "a value exactly on an edge or on a grid depth" happens often and
exactly, in float32 too."""
import math
from fractions import Fraction

import numpy as np
import pytest

import posterior_ref as R

pytestmark = pytest.mark.gpu
CHUNK = 8192       # POST_CHUNK
BLOCK = 256        # rows of a post_iface_kernel workgroup
COLKEYS = ("kmin", "kmax", "scale", "x0", "exact", "sums", "median")


def synth(rs, N, ML=21, dtype=np.float32, grid=False):
    rows = np.full((N, 2 * ML), np.nan)
    n = rs.randint(1, ML + 1, N)
    for i in range(N):
        if grid:
            rows[i, :n[i]] = rs.randint(64, 155, n[i]) / 32.
            rows[i, n[i]:2 * n[i]] = np.sort(rs.randint(0, 241, n[i])) / 4.
        else:
            rows[i, :n[i]] = rs.uniform(2.0, 4.8, n[i])
            rows[i, n[i]:2 * n[i]] = np.sort(rs.uniform(0, 60, n[i]))
    return rows.astype(dtype)


def one_layer(values, ML=2, dtype=np.float64):
    """Rows of one layer with the given vs: every column of the site is the list of values itself."""
    rows = np.full((len(values), 2 * ML), np.nan, dtype)
    rows[:, 0] = values
    rows[:, 1] = 1.0
    return rows


def deal(rs, per, nan_rows=0):
    """The sites' rows in one array in a random order, `nan_rows` NaN-only rows among them: (rows, site)."""
    rows = np.concatenate(per)
    site = np.concatenate([np.full(len(p), s, np.int32) for s, p in enumerate(per)])
    if nan_rows:
        rows = np.concatenate((rows, np.full((nan_rows, rows.shape[1]), np.nan, rows.dtype)))
        site = np.concatenate((site, rs.randint(0, len(per), nan_rows).astype(np.int32)))
    perm = rs.permutation(len(rows))
    return rows[perm], site[perm]


def grid_of(D):
    """D depths: a negative one, depths that interfaces of the grid rows equal, and one at or below every interface."""
    if D == 2:
        return np.array([-1.0, 60.0])
    return np.concatenate(([-1.0], np.arange(D - 2) * 0.5, [200.0]))


DEP65 = grid_of(65)


def kept(m):
    return int((~np.isnan(m).all(1)).sum()) if len(m) else 0


def site_ref(m, dep, public=True):
    """What the engine must return for a site that holds the rows m alone."""
    ref = dict(n=kept(m))
    if not ref["n"]:
        return ref
    vsi = R.interp(m, dep)
    scale, x0, exact = R.scale_rule(vsi)
    s1, s2 = R.int_sums(vsi, scale, x0)
    ref.update(min=vsi.min(0), max=vsi.max(0), median=R.median(vsi), scale=scale, x0=x0, exact=exact, s1=s1, s2=s2)
    if public:
        ref["mode"], _, ref["mode_valid"] = R.mode(vsi, dep)
    return ref


def load_columns(models, site, S, dep, engine):
    from bayhunter_amd.posterior import _Loaded
    ld = _Loaded(models, site, engine, nsites=S)
    try:
        col = ld.columns(dep)
    finally:
        ld.close()
    col.update(rows=ld.rows.copy(), invalid=ld.invalid.copy(), dropped=ld.dropped)
    return col


def summarise(models, site, S, dep, engine):
    from bayhunter_amd.posterior import posterior_models
    return load_columns(models, site, S, dep, engine), posterior_models(models, site=site, dep_int=dep, engine=engine, nsites=S)


def limbs(sums):
    v = [int(x) for x in sums]
    return v[0] + (v[1] << 32), v[2] + (v[3] << 32) + (v[4] << 64) + (v[5] << 96)


def check_columns(col, s, ref):
    """bh_posterior_columns of site s, every column: min, max, median, scale, x0, exact and the recombined limbs."""
    from bayhunter_amd.posterior import _keys_to_values
    n = ref["n"]
    assert col["rows"][s] == n
    D = col["scale"].shape[1]
    if not n:
        assert not col["scale"][s].any() and not col["x0"][s].any() and not col["sums"][s].any() and col["exact"][s].all()
        return
    assert np.array_equal(col["min"][s], ref["min"]) and np.array_equal(col["max"][s], ref["max"])
    assert np.array_equal(np.signbit(col["min"][s]), np.signbit(ref["min"]))
    med = _keys_to_values(col["median"][s].reshape(-1), col["keys32"]).reshape(D, 2)
    assert np.all(med[:, 0] <= med[:, 1])
    median = med[:, 0] if n % 2 else (med[:, 0] + med[:, 1]) / 2.
    assert np.array_equal(median, ref["median"])
    assert [int(v) for v in col["scale"][s]] == ref["scale"]
    assert [int(v) for v in col["x0"][s]] == ref["x0"]
    assert [int(v) for v in col["exact"][s]] == ref["exact"]
    for j in range(D):
        assert limbs(col["sums"][s, j]) == (ref["s1"][j], ref["s2"][j]), (s, j)


def check_public(col, r, s, ref):
    """posterior_models of site s, every column: count, min, max, median, mode; the mean is the correctly rounded exact mean,
    the std within 1 ulp of the exact one, stdminmax exactly mean -+ std."""
    from bayhunter_amd.posterior import _mean_std
    n = ref["n"]
    assert r["count"] == n and r["invalid_rows"] == col["invalid"][s]
    if not n:
        for k in ("mean", "median", "minmax", "stdminmax", "mode"):
            assert np.isnan(r[k][0]).all()
        assert not r["mode_valid"]
        return
    assert np.array_equal(r["minmax"][0][0], ref["min"]) and np.array_equal(r["minmax"][0][1], ref["max"])
    assert np.array_equal(r["median"][0], ref["median"])
    assert r["mode_valid"] == ref["mode_valid"]
    assert np.array_equal(r["mode"][0], ref["mode"], equal_nan=True)
    mean, (lo, hi) = r["mean"][0], r["stdminmax"][0]
    for j in range(len(mean)):
        s1, s2, L, x0 = ref["s1"][j], ref["s2"][j], ref["scale"][j], ref["x0"][j]
        assert mean[j] == float(R.exact_mean(n, s1, L, x0)), (s, j)
        m, sd = _mean_std(n, col["sums"][s, j], col["scale"][s, j], col["x0"][s, j])
        assert m == mean[j]
        want = R.exact_std(n, s1, s2, L)
        if want == 0:
            assert sd == 0.0
        else:
            assert abs(Fraction(sd) - want) <= Fraction(math.ulp(max(sd, float(want)))), (s, j, sd, float(want))
        assert lo[j] == mean[j] - sd and hi[j] == mean[j] + sd


def check_all(col, res, per, dep, refs=None):
    assert col["dropped"] == 0 and not col["invalid"].any()
    for s, m in enumerate(per):
        ref = refs[s] if refs is not None else site_ref(m, dep)
        check_columns(col, s, ref)
        check_public(col, res[s], s, ref)


def same_columns(a, b, sa=None, sb=None):
    for k in COLKEYS:
        x, y = (a[k], b[k]) if sa is None else (a[k][sa], b[k][sb])
        assert np.array_equal(x, y), k


# ---- a. load and scatter -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ML", [1, 2, 21, 32])
def test_row_widths_from_one_layer_to_the_maximum(ML, engine):
    rs = np.random.RandomState(40 + ML)
    per = [synth(rs, 150, ML=ML), synth(rs, 150, ML=ML, grid=True)]
    rows, site = deal(rs, per, nan_rows=9)
    col, res = summarise(rows, site, 2, DEP65, engine)
    check_all(col, res, per, DEP65)
    if ML == 1:                                    # constant columns, no interface
        for s in range(2):
            assert np.all(col["min"][s] == col["min"][s][0]) and np.all(res[s]["median"][0] == res[s]["median"][0][0])
            assert res[s]["mode_valid"]            # the rows differ by more than one 0.025 km/s bin


@pytest.mark.parametrize("N", [1, 255, 256, 257, 513])
def test_row_counts_around_a_workgroup_of_the_load(N, engine):
    rs = np.random.RandomState(N)
    per = [synth(rs, N, grid=bool(N % 2))]
    rows, site = deal(rs, per)
    col, res = summarise(rows, site, 1, DEP65, engine)
    check_all(col, res, per, DEP65)


def test_an_empty_site_between_two_others(engine):
    rs = np.random.RandomState(3)
    per = [synth(rs, 70), synth(rs, 0), synth(rs, 90, grid=True)]
    rows, site = deal(rs, per, nan_rows=5)
    site[np.isnan(rows).all(1)] = 1                # the NaN-only rows are the middle site's: neither kept nor counted
    col, res = summarise(rows, site, 3, DEP65, engine)
    assert list(col["rows"]) == [70, 0, 90]
    check_all(col, res, per, DEP65)


def test_64_distinct_sites_in_every_wavefront(engine):
    """130 sites dealt round robin over 257 rows: every wavefront of the load holds 64 distinct sites (agg_add loops once per
    site); then the same rows sorted by site."""
    rs = np.random.RandomState(130)
    S, N = 130, 257
    rows = synth(rs, N, grid=True)
    rows[::2] = synth(rs, N)[::2]
    rows[rs.choice(N, 6, replace=False)] = np.nan
    site = (np.arange(N) % S).astype(np.int32)
    for w in range(0, N - 63, 64):
        assert len(set(site[w:w + 64])) == 64
    per = [rows[site == s] for s in range(S)]
    refs = [site_ref(m, DEP65) for m in per]
    col, res = summarise(rows, site, S, DEP65, engine)
    check_all(col, res, per, DEP65, refs)
    order = np.argsort(site, kind="stable")
    col2, res2 = summarise(rows[order], site[order], S, DEP65, engine)
    check_all(col2, res2, per, DEP65, refs)
    same_columns(col, col2)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_rows_with_a_wide_stride_bad_rows_and_bad_sites(dtype, engine):
    import torch
    rs = np.random.RandomState(77)
    S, ML, N = 3, 6, 900
    good = synth(rs, N, ML=ML, dtype=dtype)
    good[::3] = synth(rs, N, ML=ML, dtype=dtype, grid=True)[::3]
    good[rs.choice(N, 20, replace=False)] = np.nan                       # NaN-only rows
    site = rs.randint(0, S, N).astype(np.int32)
    wide = np.empty((N, 2 * ML + 5), dtype)
    wide[:, :2 * ML] = good
    wide[:, 2 * ML:] = rs.uniform(-9, 9, (N, 5))                         # the gap: finite garbage ...
    wide[::2, 2 * ML:] = np.nan                                          # ... or NaN
    nlay = (~np.isnan(good)).sum(1) // 2
    free = np.flatnonzero((nlay >= 2) & (nlay < ML))
    pick = rs.choice(free, 90, replace=False)
    odd, hole, out = pick[:30], pick[30:60], pick[60:]
    wide[odd, 2 * nlay[odd]] = 1.0                                       # an odd number of values
    wide[hole, 1] = np.nan                                               # a NaN hole
    site[out[:15]], site[out[15:]] = -1, S                               # sites out of range
    site[odd[:3]] = -1                                                   # (a bad row of a bad site is dropped, not invalid)
    bad = np.zeros(N, bool)
    bad[odd], bad[hole] = True, True
    inside = (site >= 0) & (site < S)
    mt = torch.from_numpy(wide).cuda()[:, :2 * ML]
    assert mt.stride(0) == 2 * ML + 5
    st = torch.from_numpy(site).cuda()
    col, res = summarise(mt, st, S, DEP65, engine)
    assert col["dropped"] == int((~inside).sum()) == 33
    for s in range(S):
        assert col["invalid"][s] == int((bad & (site == s)).sum()) > 0
        ref = site_ref(good[~bad & (site == s)], DEP65)
        check_columns(col, s, ref)
        check_public(col, res[s], s, ref)


# ---- b. column passes ----------------------------------------------------------------------------------------------------------

SIZES = (1, 2, 3, 64, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
KINDS = ("f32", "f64of32", "f64")


class Eight(object):
    """One load of 8 sites around the chunk size, the input order permuted; the odd sites hold grid rows.  The references are
    computed once per (kind, site, grid) and shared."""

    def __init__(self):
        rs = np.random.RandomState(8192)
        self.per32 = [synth(rs, n, grid=bool(s % 2)) for s, n in enumerate(SIZES)]
        self.noise = [rs.uniform(-1e-7, 1e-7, p.shape) for p in self.per32]
        self.site = np.concatenate([np.full(n, s, np.int32) for s, n in enumerate(SIZES)])
        self.perm = rs.permutation(len(self.site))
        self._ref = {}

    def site_rows(self, kind, s):
        m = self.per32[s]
        return m if kind == "f32" else m.astype(np.float64) if kind == "f64of32" else m.astype(np.float64) + self.noise[s]

    def rows(self, kinds):
        per = [self.site_rows(k, s) for s, k in enumerate(kinds)]
        return np.concatenate(per)[self.perm], self.site[self.perm], per

    def ref(self, kind, s, D):
        if (kind, s, D) not in self._ref:
            self._ref[kind, s, D] = site_ref(self.site_rows(kind, s), grid_of(D))
        return self._ref[kind, s, D]


@pytest.fixture(scope="module")
def eight():
    return Eight()


@pytest.mark.parametrize("D", [2, 64, 65, 129])
@pytest.mark.parametrize("kind", KINDS)
def test_columns_of_sites_around_the_chunk_size(eight, kind, D, engine):
    rows, site, per = eight.rows([kind] * 8)
    dep = grid_of(D)
    col, res = summarise(rows, site, 8, dep, engine)
    assert col["keys32"] == (kind != "f64")
    assert list(col["rows"]) == list(SIZES)
    if kind != "f64" and D > 2:                     # interfaces of the grid rows lie exactly on grid depths (the <= of `sample`)
        assert np.isin(R.depths(per[7])[1], dep).sum() >= 50
    if kind == "f64":                               # the limbs s1, q2, q3 are in use: all six are non-zero somewhere
        assert (col["sums"] != 0).all(-1).any()
    else:
        assert not col["sums"][..., (1, 4, 5)].any()
    check_all(col, res, per, dep, [eight.ref(kind, s, D) for s in range(8)])


def test_one_site_of_general_float64_values_among_float32_ones(eight, engine):
    kinds = ["f64of32"] * 8
    kinds[3] = "f64"
    rows, site, per = eight.rows(kinds)
    col, res = summarise(rows, site, 8, DEP65, engine)
    assert not col["keys32"]
    assert (col["sums"][3] != 0).all(-1).any() and not np.delete(col["sums"], 3, 0)[..., (1, 4, 5)].any()
    check_all(col, res, per, DEP65, [eight.ref(k, s, 65) for s, k in enumerate(kinds)])


def test_ties_across_chunks_and_the_two_middle_values(engine):
    a = 3.3
    b = float(np.nextafter(a, 4.0))
    c = 3.5
    assert (np.float64(a).view(np.uint64) & np.uint64(0xff)) % 2 == 0    # a and b: the two halves of one packed counter pair
    sets = [[a] * (CHUNK + 1),                    # identical rows over two chunks
            [a] * 4096 + [b] * 4097,              # one ulp apart: the last radix pass decides
            [a] * 4097 + [b] * 4096,
            [a, b], [a, a], [a, b, b, c], [a, a, b, b], [a, b, c, c],
            [a] * 4096 + [b] * 4096,              # even, the middle values differ
            [a] * 4096 + [b] * 4098,              # even, the middle values are equal, over two chunks
            [a] * 4097 + [b] * 4097]              # even, the middle values differ, over two chunks
    rs = np.random.RandomState(12)
    per = [one_layer(v) for v in sets]
    rows, site = deal(rs, per)
    dep = np.array([-1.0, 0.5, 3.0])
    col, res = summarise(rows, site, len(per), dep, engine)
    assert not col["keys32"]
    check_all(col, res, per, dep)
    want = [a, b, a, (a + b) / 2., a, b, (a + b) / 2., (b + c) / 2., (a + b) / 2., b, (a + b) / 2.]
    assert [r["median"][0][0] for r in res] == want
    # the same ties in multi-layer float32 rows: columns of few distinct values across a chunk boundary
    rs = np.random.RandomState(13)
    m = synth(rs, 2 * CHUNK, ML=3, grid=True)
    m[:, :3] = np.where(np.isnan(m[:, :3]), np.nan, rs.randint(96, 99, (len(m), 3)) / 32.).astype(np.float32)
    per = [m[:CHUNK + 2], m[CHUNK + 2:]]
    rows, site = deal(rs, per)
    col, res = summarise(rows, site, 2, DEP65, engine)
    assert col["keys32"]
    check_all(col, res, per, DEP65)


def test_zero_columns_the_sign_of_the_keys_and_a_raised_scale(engine):
    rs = np.random.RandomState(14)
    zeros = np.full((40, 4), np.nan)
    zeros[:, :2], zeros[:, 2], zeros[:, 3] = 0.0, 1.0, 3.0               # two layers, vs 0.0: amax == 0
    signed = synth(rs, 300, ML=4, dtype=np.float64)
    signed[:, :4] = np.where(np.isnan(signed[:, :4]), np.nan, rs.uniform(-1, 1, (300, 4)))
    assert not (signed[:, :4] == 0).any()
    raised = one_layer(rs.choice([4.0, 2.0 ** -70, 2.75, 3 * 2.0 ** -70], 50), ML=4)
    per = [np.concatenate((zeros, np.full((40, 4), np.nan)), axis=1), signed, raised]
    rows, site = deal(rs, per)
    dep = grid_of(64)
    col = load_columns(rows, site, 3, dep, engine)
    refs = [site_ref(m, dep, public=False) for m in per]
    for s in range(3):
        check_columns(col, s, refs[s])
    assert not col["scale"][0].any() and col["exact"][0].all() and not col["sums"][0].any()
    assert (col["min"][1] < 0).all() and (col["max"][1] > 0).all()
    assert not col["exact"][2].any() and np.all(col["scale"][2] == -59)
    vsi = R.interp(per[2], dep)
    X = [[int(x) for x in np.rint(np.ldexp(vsi[:, j], 59))] for j in range(64)]
    for j in range(64):
        assert limbs(col["sums"][2, j]) == (sum(X[j]), sum(x * x for x in X[j]))   # x0 = rint(2^-70 2^59) = 0
    s32 = signed.astype(np.float32)                                       # ... and the 32-bit keys across the sign
    col = load_columns(s32, np.zeros(300, np.int32), 1, dep, engine)
    assert col["keys32"]
    check_columns(col, 0, site_ref(s32, dep, public=False))


# ---- c. histogram and argmax -------------------------------------------------------------------------------------------------

def vs_edges(rs, nb, lo=2.5, hi=4.0):
    """nb + 1 ascending dyadic edges from lo to hi, narrower than the data: points of the 1/32 grid, then of a 1/1024 grid."""
    base = np.arange(lo * 32 + 1, hi * 32) / 32.
    if nb - 1 <= base.size:
        inner = rs.choice(base, nb - 1, replace=False)
    else:
        fine = np.setdiff1d(np.arange(lo * 1024 + 1, hi * 1024) / 1024., base)
        inner = np.concatenate((base, rs.choice(fine, nb - 1 - base.size, replace=False)))
    return np.concatenate(([lo], np.sort(inner), [hi]))


def on_edges(v, e):
    """How many values lie on an inner edge, on the last edge, below the first edge and above the last."""
    return (int(np.isin(v, e[1:-1]).sum()), int((v == e[-1]).sum()), int((v < e[0]).sum()), int((v > e[-1]).sum()))


def layouts():
    """D = 130 samples and their depth bins: (samples, depth edges)."""
    half = np.arange(130) * 0.5
    return dict(plot=(half, np.arange(0, 71, 1.0)),               # two samples per bin; the bins below 65 km hold none
                outside=(half - 2.0, np.arange(0, 61, 1.0)),      # samples above the first and below the last bin
                one=(half, np.array([10.0, 20.0])))               # ND = 1


class HistLoad(object):
    """One load of six sites -- 700 plain rows, 8193 grid rows, 8192 identical rows, one row, none, and two one-layer rows whose
    bins tie -- with three sets of per-site edge tables (bin counts BINS: every site at most 256 bins, one site above, odd
    counts) and three depth layouts.  The references are computed once and shared."""
    BINS = dict(lds=(1, 255, 256, 2, 2, 4), glob=(1, 257, 256, 300, 2, 4), odd=(255, 256, 255, 1, 255, 4))

    def __init__(self):
        rs = np.random.RandomState(256)
        self.per = [synth(rs, 700), synth(rs, CHUNK + 1, grid=True), np.repeat(synth(rs, 1, grid=True), CHUNK, axis=0),
                    synth(rs, 1, grid=True), synth(rs, 0), one_layer([2.75, 3.5], ML=21, dtype=np.float32)]
        self.per[2][:, :21] = np.where(np.isnan(self.per[2][:, :21]), np.nan, np.float32(2.5 + 123 / 1024.))
        self.rows, self.site = deal(rs, self.per, nan_rows=4)
        self.edges = {k: [vs_edges(rs, nb) for nb in v] for k, v in self.BINS.items()}
        self.edges["glob"][0], self.edges["glob"][2] = self.edges["lds"][0], self.edges["lds"][2]
        self.edges["odd"][5] = self.edges["glob"][5] = self.edges["lds"][5] = np.array([2.5, 2.75, 3.0, 3.5, 4.0])
        self.layouts = layouts()
        self._vsi, self._ref = {}, {}

    def vsi(self, s, lay):
        if (s, lay) not in self._vsi:
            m = self.per[s]
            self._vsi[s, lay] = R.interp(m, self.layouts[lay][0]) if kept(m) else np.zeros((0, 130))
        return self._vsi[s, lay]

    def ref(self, s, lay, which):
        if (s, lay, which) not in self._ref:
            samples, de = self.layouts[lay]
            self._ref[s, lay, which] = R.hist2d(self.vsi(s, lay), samples, self.edges[which][s], de)
        return self._ref[s, lay, which]


@pytest.fixture(scope="module")
def histload():
    return HistLoad()


def run_hist(H, lay, which, engine, rows=None, site=None, S=6, edges=None):
    from bayhunter_amd.posterior import _Loaded, depth_bins
    samples, de = H.layouts[lay]
    ld = _Loaded(H.rows if rows is None else rows, H.site if site is None else site, engine, nsites=S)
    try:
        return ld.hist(samples, depth_bins(samples, de), de.size - 1, H.edges[which] if edges is None else edges, argmax=True)
    finally:
        ld.close()


@pytest.mark.parametrize("lay", ["plot", "outside", "one"])
def test_histogram_counts_of_per_site_edge_tables_on_both_paths(histload, lay, engine):
    from bayhunter_amd.posterior import depth_bins
    H = histload
    samples, de = H.layouts[lay]
    dbin = depth_bins(samples, de)
    assert (dbin < 0).any() == (lay != "plot") and dbin.max() == {"plot": 64, "outside": 59, "one": 0}[lay]
    e = H.edges["lds"][2]                              # the site of identical rows: one half-counter takes them all
    b = int(R.hist_bins(np.array([2.5 + 123 / 1024.]), e)[0])
    assert b >= 0
    for which in ("lds", "glob"):                      # values on inner edges, on the last edge and outside, on both paths
        assert min(on_edges(H.vsi(1, lay)[:, dbin >= 0], H.edges[which][1])) >= 50
    got = {}
    for which in ("lds", "glob", "odd"):
        assert (max(H.BINS[which]) <= 256) == (which != "glob")
        counts, am = got[which] = run_hist(H, lay, which, engine)
        total = 0
        for s in range(6):
            want = H.ref(s, lay, which)
            assert counts[s].shape == want.shape and np.array_equal(counts[s], want), (which, s)
            assert np.array_equal(am[s], np.argmax(want, axis=0)), (which, s)
            v, ed = H.vsi(s, lay)[:, dbin >= 0], H.edges[which][s]
            total += int(((v >= ed[0]) & (v <= ed[-1])).sum())
        assert sum(int(c.sum(dtype=np.int64)) for c in counts) == total
        assert not counts[4].any() and not am[4].any()               # the site without rows
        two = H.ref(5, lay, which)                                   # the two-row site: two bins tie, the first wins
        tie = ((two == two.max(0)) & (two > 0)).sum(0)
        assert tie.max() == 2 and np.all(am[5][tie == 2] == 1)
        if lay == "plot":
            assert not np.array(H.ref(1, lay, which))[:, 65:].any() and not am[1][65:].any()   # depth bins without a sample
    ident = got["lds"][0][2]
    per_bin = np.bincount(dbin[dbin >= 0], minlength=de.size - 1)     # every sample of a depth bin brings one full half-counter
    assert np.array_equal(ident[b], CHUNK * per_bin) and (ident.sum(0) == ident[b]).all()
    for s in (0, 2, 5):                                # the same edges in both calls: the same counts on both paths
        assert np.array_equal(got["lds"][0][s], got["glob"][0][s])


@pytest.mark.parametrize("given", [False, True])
def test_public_hist2d_of_several_sites(histload, given, engine):
    from bayhunter_amd.posterior import posterior_hist2d, hist2d_edges
    H = histload
    kw = dict(vs_edges=H.edges["odd"][0], dep_edges=np.arange(2.0, 40.5, 0.5)) if given else {}
    got = posterior_hist2d(H.rows, site=H.site, nsites=6, engine=engine, **kw)
    samples, depbins, _ = hist2d_edges(None, None, None)
    depbins = kw.get("dep_edges", depbins)
    for s, m in enumerate(H.per):
        g = got[s]
        assert g["count"] == kept(m) and np.array_equal(g["samples"], samples) and np.array_equal(g["dep_edges"], depbins)
        if not kept(m):
            assert not g["counts"].any() and not g["interfaces"].any()
            continue
        vsi = R.interp(m, samples)
        vse = kw["vs_edges"] if given else hist2d_edges(vsi.min(), vsi.max(), None)[2]
        assert np.array_equal(g["vs_edges"], vse)
        assert np.array_equal(g["counts"], R.hist2d(vsi, samples, vse, depbins)), s
        assert np.array_equal(g["interfaces"], R.interface_hist(m, depbins)), s


# ---- d. interfaces -------------------------------------------------------------------------------------------------------------

IFACE_SIZES = (300, 100, 100, 100, 0, 1, 700)
LAST_EDGE = 37.5


def iface_rows(kind):
    """Seven sites, the odd ones of grid rows; rows of one layer, rows with three nuclei at one depth and rows whose last
    interface is LAST_EDGE among them."""
    rs = np.random.RandomState(700)
    per = []
    for s, n in enumerate(IFACE_SIZES):
        m = synth(rs, n, grid=s % 2 == 1)
        noise = rs.uniform(-1e-7, 1e-7, m.shape)
        if kind != "f32":
            m = m.astype(np.float64) + (noise if kind == "f64" and s % 2 == 0 else 0.0)
        nlay = (~np.isnan(m)).sum(1) // 2
        for i in np.flatnonzero(nlay >= 4)[::5]:
            m[i, nlay[i] + 1:nlay[i] + 4] = m[i, nlay[i] + 2]        # three nuclei at one depth: two equal interface depths
        for i in np.flatnonzero(nlay >= 2)[::3]:
            k = nlay[i]
            if k == 2 or m[i, 2 * k - 3] <= LAST_EDGE:
                m[i, 2 * k - 2:2 * k] = LAST_EDGE                    # the deepest interface on the last edge
        m[::11] = np.nan
        m[::11, 0], m[::11, 1] = 3.0, 7.0                            # rows of one layer: no interface
        per.append(m)
    rows, site = deal(rs, per, nan_rows=7)
    return per, rows, site


def iface_depths(per):
    di = np.concatenate([R.depths(m)[2].ravel() for m in per if len(m)]).astype(np.float64)
    return di[~np.isnan(di)]


def iface_edges(per, nb, lo=2.0, hi=LAST_EDGE):
    """nb + 1 ascending edges from lo to hi: points of the 0.125 grid, then interface depths of the rows themselves (an interface
    whose running sum came out one bit lower would leave its bin), then points of a 1/4096 grid."""
    rs = np.random.RandomState(nb)
    base = np.arange(lo * 8 + 1, hi * 8) / 8.
    if nb - 1 <= base.size:
        inner = rs.choice(base, nb - 1, replace=False)
    else:
        di = iface_depths(per)
        own = np.setdiff1d(di[(di > lo) & (di < hi)], base)
        need = nb - 1 - base.size
        if own.size < need:
            fine = np.setdiff1d(np.arange(lo * 4096 + 1, hi * 4096) / 4096., np.concatenate((base, own)))
            own = np.concatenate((own, rs.choice(fine, need - own.size, replace=False)))
        inner = np.concatenate((base, rs.choice(own, need, replace=False)))
    return np.concatenate(([lo], np.sort(inner), [hi]))


def block_spans(sizes):
    """How many sites every 256-row workgroup of post_iface_kernel meets, from the site sizes (the slices lie in site order)."""
    off = np.concatenate(([0], np.cumsum(sizes)))
    n = int(off[-1])
    return [len(np.unique(np.searchsorted(off, np.arange(b, min(b + BLOCK, n)), side="right"))) for b in range(0, n, BLOCK)], n


@pytest.mark.parametrize("nb", [1, 4096, 4097])
@pytest.mark.parametrize("kind", KINDS)
def test_interface_counts_on_the_shared_and_the_global_counters(kind, nb, engine):
    from bayhunter_amd.posterior import _Loaded
    per, rows, site = iface_rows(kind)
    edges = iface_edges(per, nb)
    spans, nrows = block_spans([kept(m) for m in per])
    assert spans[0] == 1 and max(spans) >= 3 and nrows % BLOCK         # a block inside one site, blocks over several, a partial one
    assert min(on_edges(iface_depths(per), edges)[0 if nb > 1 else 1:]) >= 50   # on inner edges, on the last edge, outside on both sides
    vs, d, dd, n = R.depths(per[0])
    assert ((n == 1).sum() > 10) and (np.diff(dd, axis=1) == 0).sum() >= 10
    ld = _Loaded(rows, site, engine, nsites=7)
    try:
        got, again = ld.interfaces(edges), ld.interfaces(edges)
    finally:
        ld.close()
    assert list(ld.rows) == [kept(m) for m in per]
    for s, m in enumerate(per):
        want = R.interface_hist(m, edges) if kept(m) else np.zeros(nb, np.int64)
        assert np.array_equal(got[s], want), s
    assert np.array_equal(got, again)
    ld = _Loaded(per[6], None, engine)                                  # a site among others equals the site loaded alone
    try:
        assert np.array_equal(ld.interfaces(edges)[0], got[6])
    finally:
        ld.close()


# ---- e. independence and repeatability ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_columns_repeat_and_equal_the_site_loaded_alone(eight, kind, engine):
    rows, site, per = eight.rows([kind] * 8)
    a = load_columns(rows, site, 8, DEP65, engine)
    b = load_columns(rows, site, 8, DEP65, engine)
    same_columns(a, b)
    for s in (2, 3, 6, 7):
        alone = load_columns(per[s], None, 1, DEP65, engine)
        assert alone["keys32"] == a["keys32"]
        same_columns(a, alone, s, 0)


def test_histograms_repeat_and_equal_the_site_loaded_alone(histload, engine):
    H = histload
    for which in ("lds", "glob"):
        a, b = run_hist(H, "outside", which, engine), run_hist(H, "outside", which, engine)
        for s in range(6):
            assert np.array_equal(a[0][s], b[0][s])
        assert np.array_equal(a[1], b[1])
        for s in (1, 2, 5):
            alone = run_hist(H, "outside", which, engine, rows=H.per[s], site=np.zeros(len(H.per[s]), np.int32), S=1,
                             edges=[H.edges[which][s]])
            assert np.array_equal(alone[0][0], a[0][s]) and np.array_equal(alone[1][0], a[1][s])
