"""DeviceChains without a GPU (bayhunter_amd/device_chains.py): the run plan `plan_chains` computes as a value -- sizes, site tables,
ladders and every refusal --, the pure pieces cut out of the constructor (`merge_noisepriors`, `initial_state_arrays`,
`_host_rows`), the one settings scope of the engine (`Engine.settings`) on a library that only counts its calls, and the
names other modules import from device_chains."""
import math
import types

import numpy as np
import pytest

from conftest import golden
import bayhunter_amd as bh
from bayhunter_amd import engine as E
from bayhunter_amd import device_chains as DC
from bayhunter_amd.device_chains import DeviceChains, initial_state_arrays, merge_noisepriors, plan_chains
from bayhunter_amd.sites import SiteTargets
from test_ellip_fused_host import ell_target
from test_sites_missing_host import slots_of
from test_sites_x_host import X_FULL, X_SETS


@pytest.fixture(scope="module")
def g():
    return golden("chain_golden.npz")


@pytest.fixture(scope="module")
def jt(g):
    return bh.JointTarget(slots_of(g, X_FULL))


def sites_of(g, have):
    return SiteTargets([slots_of(g, X_SETS[s % 2], 0.01 * s, h) for s, h in enumerate(have)], per_site_x="all", missing=True)


# ---- plan_chains: the sizes ---------------------------------------------------------------------------------------------------------

def depth_of(C, spec_depth):
    """the deepest tree of at most 7 levels whose C (2^d - 1) nodes stay within 1024 evaluations, at least 1"""
    if spec_depth is not None:
        return spec_depth
    return max([1] + [d for d in range(1, 8) if C * (2 ** d - 1) <= 1024])


@pytest.mark.parametrize("nchains", [1, 8, 64])
@pytest.mark.parametrize("spec_depth", [None, 1, 7])
@pytest.mark.parametrize("iter_main, maxmodels", [(40, 40), (100, 40)])
def test_plan_sizes(g, jt, monkeypatch, nchains, spec_depth, iter_main, maxmodels):
    monkeypatch.delenv("BH_SPEC_BUDGET", raising=False)
    ip = dict(iter_burnin=30, iter_main=iter_main, maxmodels=maxmodels)
    thinning = {(40, 40): 1, (100, 40): 3}[iter_main, maxmodels]
    assert thinning == max(1, math.ceil(iter_main / maxmodels))
    # one station
    p = plan_chains(jt, nchains, ip, dict(layers=(1, 12)), spec_depth=spec_depth)
    d = depth_of(nchains, spec_depth)
    assert (p.nsites, p.C_site, p.C, p.nt, p.site_ML, p.ML) == (1, nchains, nchains, 3, [13], 13)
    assert (p.iter_phase1, p.iter_phase2, p.iterations, p.thinning) == (30, iter_main, 30 + iter_main, thinning)
    assert (p.depth, p.ld) == (d, nchains * (2 ** d - 1))
    assert p.present is None and p.site_map is None and p.absent is None and p.ladder is None and not p.prior_table
    assert (p.record, p.ladder_adapt, p.search, p.arith) == ("host", None, "fast", "fast")
    assert p.site_initparams[0]["iter_main"] == iter_main and p.site_priors[0]["layers"] == (1, 12)
    assert plan_chains(slots_of(g, X_FULL)[:2], nchains, ip).nt == 2              # a plain list of targets
    # two sites with different layers maxima: the arrays have the rows of the larger, the table of priors is in use
    st = SiteTargets([slots_of(g, X_SETS[0]), slots_of(g, X_SETS[1], 0.01)], per_site_x="all")
    p = plan_chains(st, nchains, ip, [dict(layers=(1, 9)), dict(layers=(2, 17))], spec_depth=spec_depth, record="device", search=None,
                    arith="exact")
    C = 2 * nchains
    d = depth_of(C, spec_depth)
    assert (p.nsites, p.C_site, p.C, p.nt, p.site_ML, p.ML) == (2, nchains, C, 3, [10, 18], 18) and p.ML == max(p.site_ML)
    assert (p.depth, p.ld, p.thinning) == (d, C * (2 ** d - 1), thinning)
    assert p.prior_table and (p.record, p.search, p.arith) == ("device", None, "exact")
    assert p.present is None and p.absent is None                                  # (no missing=True)
    want = (np.arange(p.ld) % C) // nchains                                        # node j of chain c in column j*C + c
    assert p.site_map.dtype == np.int32 and np.array_equal(p.site_map, want)
    assert not plan_chains(st, nchains, ip, dict(layers=(1, 9))).prior_table and plan_chains(st, nchains, ip, prior_table=True).prior_table
    with pytest.raises(AttributeError):
        p.depth = 2                                                                # a value


def test_plan_refusals_keep_their_messages_and_their_order(g, jt):
    st = sites_of(g, ["111", "111"])
    B4 = np.array([1.0, 0.7, 0.4, 0.1])
    with pytest.raises(ValueError, match="record must be 'host' or 'device', not 'gpu'"):
        plan_chains(None, 4, record="gpu", ladder_adapt="on")                      # first of all: no targets are looked at
    with pytest.raises(ValueError, match=r"ladder_adapt: unknown key 'evry' \(known: \['every', 'lag', 'rate'\]\)"):
        plan_chains(None, 4, betas=B4, swap_every=5, ladder_adapt=dict(evry=4))
    with pytest.raises(E.EngineError, match=r"DeviceChains does not run RayleighEllipticity: the device chains evaluate engine-backed "
                                            r"targets in one fused call, and the ellipticity is not part of it yet \(ChainBatch runs it\)"):
        plan_chains([ell_target(fused=False)], 4, modelpriors=[{}], search="x")    # ... before the dicts and the options
    assert plan_chains([ell_target()], 4, modelpriors={"ellnoise_corr": 0.0, "ellnoise_sigma": (0.01, 0.2)}).nt == 1
    with pytest.raises(ValueError, match="a sequence of modelpriors dicts needs SiteTargets"):
        plan_chains(jt, 4, modelpriors=[{}], prior_table=True)
    with pytest.raises(ValueError, match="prior_table=True needs SiteTargets"):
        plan_chains(jt, 4, prior_table=True, search="x")
    with pytest.raises(E.EngineError, match="DeviceChains with SiteTargets does not shard: give each process its own sites instead of dist"):
        plan_chains(st, 4, dist=object(), search="x")
    with pytest.raises(ValueError, match="search must be None, 'reference', 'fast' or 'fast_rayleigh'"):
        plan_chains(jt, 4, search="exact", arith="x")
    with pytest.raises(ValueError, match="arith must be None, 'exact' or 'fast'"):
        plan_chains(jt, 4, arith="reference", spec_depth=0)
    for bad in (0, 8, -1):
        with pytest.raises(E.EngineError, match=r"spec_depth must be 1\.\.7"):
            plan_chains(jt, 4, spec_depth=bad)
    # the constructor reports them as they are, before it asks for an engine (this test runs without a GPU)
    for kw, exc, what in ((dict(search="exact"), ValueError, "search must be"), (dict(arith="x"), ValueError, "arith must be"),
                          (dict(spec_depth=8), E.EngineError, "spec_depth must be"), (dict(prior_table=True), ValueError, "needs SiteTargets")):
        with pytest.raises(exc, match=what):
            DeviceChains(jt, 4, **kw)
    with pytest.raises(E.EngineError, match="spans sites"):
        DeviceChains(st, 2, betas=B4, ladder=[0, 0, 0, 1], swap_every=5)


def test_plan_absent_bits_and_present(g):
    st = sites_of(g, ["111", "101", "111"])
    present = np.array([[True, True, True], [True, False, True], [True, True, True]])
    assert np.array_equal(st.present, present)
    p = plan_chains(st, 5, spec_depth=2)
    bits = [sum(int(not present[s, t]) << t for t in range(3)) for s in range(3)]
    assert bits == [0, 2, 0]
    assert p.absent.dtype == np.uint8 and np.array_equal(p.absent, np.repeat(bits, 5)) and np.array_equal(p.present, present)
    assert (p.C_site, p.C, p.nt, p.ld) == (5, 15, 3, 45) and np.array_equal(p.site_map, np.tile(np.repeat([0, 1, 2], 5), 3))
    assert plan_chains(sites_of(g, ["110", "011"]), 1).absent.tolist() == [4, 1]


def test_plan_ladders_lie_within_sites(g, jt):
    st = sites_of(g, ["111", "111"])
    betas = np.tile([1.0, 0.5, 1.0, 0.5], 2)
    with pytest.raises(E.EngineError, match="tempering ladder 1 spans sites: every ladder must lie within one site"):
        plan_chains(st, 4, betas=betas, ladder=[0, 0, 1, 1, 1, 1, 2, 2], swap_every=5)
    p = plan_chains(st, 4, betas=betas, ladder=[0, 0, 1, 1, 2, 2, 3, 3], swap_every=5)
    assert p.ladder.dtype == np.int64 and p.ladder.tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    assert plan_chains(st, 4, ladder=[0] * 8).ladder is None                       # untempered: no ladders
    with pytest.raises(E.EngineError, match="tempering ladder 0 spans sites"):
        plan_chains(st, 4, betas=betas, swap_every=5)                              # the default: one ladder of all chains
    betas = 1.0 / np.geomspace(1.0, 8.0, 8)
    p = plan_chains(jt, 8, betas=betas, swap_every=5, ladder_adapt={"every": 2})   # one station: one ladder of all chains is fine
    assert p.ladder.tolist() == [0] * 8 and p.ladder_adapt == dict(every=2, rate=0.5, lag=50.0)


# ---- the pieces cut out of the constructor ------------------------------------------------------------------------------------------

def test_merge_noisepriors_three_branches():
    a, b = [0.0, (1e-5, 0.1), (0.3, 0.7), (1e-5, 0.05)], [0.0, (1e-5, 0.2), (0.3, 0.7), (1e-5, 0.05)]
    # every slot everywhere, no table: the one list, or "differ"
    assert merge_noisepriors([a, list(a), list(a)], None, 2, False) == (a, None)
    with pytest.raises(E.EngineError, match="^the sites' noise priors differ$"):
        merge_noisepriors([a, list(a), b], None, 2, False)
    # missing slots, no table: slot by slot among the sites that have the slot
    present = np.array([[True, False], [True, True], [False, True]])
    own = [a[:2], a, a[2:]]
    assert merge_noisepriors(own, present, 2, False) == (a, None)
    assert merge_noisepriors([a[:2], a[:2]], np.array([[True, False], [True, False]]), 2, False) == (a[:2] + [None, None], None)
    with pytest.raises(E.EngineError, match="^the sites' noise priors differ$"):
        merge_noisepriors([b[:2], a, a[2:]], present, 2, False)
    with pytest.raises(E.EngineError, match="differ"):
        merge_noisepriors([a[:2], a, [(0.3, 0.7), 0.01]], present, 2, False)
    # the table: one row per site in the slot layout, nothing compared; a slot the site lacks is fixed at 0
    assert merge_noisepriors([a, b], None, 2, True) == (None, [a, b])
    assert merge_noisepriors([b[:2], a, b[2:]], present, 2, True) == (None, [b[:2] + [0.0, 0.0], a, [0.0, 0.0] + b[2:]])


def fake_chain(rs, n, k):
    """what initial_state_arrays reads of a host chain: n layers, k targets"""
    return types.SimpleNamespace(currentmodel=np.concatenate((rs.uniform(2, 5, n), np.sort(rs.uniform(0, 60, n)))),
                                 currentnoise=rs.uniform(0, 1, 2 * k), currentmisfits=rs.uniform(0, 1, k + 1),
                                 currentlikelihood=rs.normal(), currentvpvs=rs.uniform(1.4, 2.1), propdist=rs.uniform(0, 0.1, 5))


@pytest.mark.parametrize("missing", [False, True])
def test_initial_state_arrays(missing):
    rs = np.random.RandomState(3)
    ML, nt, C_site, layers = 6, 3, 2, [2, 3, 3, 5]
    present = np.array([[True, True, True], [True, False, True]]) if missing else None
    chains = [fake_chain(rs, n, 3 if present is None else int(present[c // C_site].sum())) for c, n in enumerate(layers)]
    a = initial_state_arrays(chains, ML, nt, present, C_site)
    assert list(a) == ["n", "vs", "z", "noise", "misfits", "like", "vpvs", "propdist"]
    assert a["n"].dtype == np.int32 and all(a[k].dtype == np.float64 for k in a if k != "n")
    assert [a[k].shape for k in a] == [(4,), (6, 4), (6, 4), (6, 4), (4, 4), (4,), (4,), (5, 4)]
    for c, ch in enumerate(chains):
        n = layers[c]
        assert a["n"][c] == n and a["like"][c] == ch.currentlikelihood and a["vpvs"][c] == ch.currentvpvs
        for i in range(ML):
            assert a["vs"][i, c] == (ch.currentmodel[i] if i < n else 0.0) and a["z"][i, c] == (ch.currentmodel[n + i] if i < n else 0.0)
        for i in range(5):
            assert a["propdist"][i, c] == ch.propdist[i]
        have = [t for t in range(nt) if present is None or present[c // C_site, t]]
        for t in range(nt):
            j = have.index(t) if t in have else None
            for k in (0, 1):
                assert a["noise"][2 * t + k, c] == (0.0 if j is None else ch.currentnoise[2 * j + k])
            assert a["misfits"][t, c] == (0.0 if j is None else ch.currentmisfits[j])
        assert a["misfits"][nt, c] == ch.currentmisfits[-1]                        # the joint misfit stays last


def test_host_rows_have_the_reference_layout():
    ML, nt, C = 4, 2, 3
    rs = np.random.RandomState(5)
    n = np.array([1, ML, 2], dtype=np.int32)
    snaps = []
    for i in range(2):
        vs, z = rs.uniform(2, 5, (ML, C)).astype(np.float32), rs.uniform(0, 60, (ML, C)).astype(np.float32)
        snaps.append(dict(n=n, vs=vs, z=z, like=rs.normal(size=C).astype(np.float32), vpvs=rs.uniform(1.4, 2, C).astype(np.float32),
                          misfits=rs.uniform(0, 1, (nt + 1, C)).astype(np.float32), noise=rs.uniform(0, 1, (2 * nt, C)).astype(np.float32),
                          beta=None))
    out = DC._host_rows(snaps, C, ML, nt)
    assert sorted(out) == ["likes", "misfits", "models", "noise", "vpvs"] and out["models"].shape == (2, C, 2 * ML)
    for i, s in enumerate(snaps):
        for c in range(C):
            want = np.concatenate((s["vs"][:n[c], c], s["z"][:n[c], c], np.full(2 * (ML - n[c]), np.nan)))   # [vs_1..vs_n, z_1..z_n, NaN..]
            assert np.array_equal(out["models"][i, c], want.astype(np.float32), equal_nan=True)
            assert out["likes"][i, c] == s["like"][c] and out["vpvs"][i, c] == s["vpvs"][c]
            assert np.array_equal(out["misfits"][i, c], s["misfits"][:, c]) and np.array_equal(out["noise"][i, c], s["noise"][:, c])
    assert not np.isnan(out["models"][:, 1]).any() and np.isnan(out["models"][:, 0, 2:]).all()
    for s in snaps:
        s["beta"] = np.array([1.0, 0.5, 0.25])
    assert np.array_equal(DC._host_rows(snaps, C, ML, nt)["beta"], [[1.0, 0.5, 0.25]] * 2)
    assert DC._host_rows([], C, ML, nt)["models"].shape == (0, C, 2 * ML)


# ---- Engine.settings on a library that counts ---------------------------------------------------------------------------------------

class CountingLibrary(object):
    """stands for Engine._L: every bh_* call is written down; getters return the stored value, everything else 0 (BH_OK)"""

    def __init__(self, search=E.SEARCH_FAST, arith=E.ARITH_FAST, trials=0):
        self.values = dict(search=search, arith=arith, trials=trials, typical_layers=0)
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("bh_"):
            raise AttributeError(name)

        def call(handle, *args):
            self.calls.append((name[len("bh_engine_"):],) + args)
            what = name.split("_swd_")[-1] if "_swd_" in name else name[len("bh_engine_set_"):]
            if "_get_" in name:
                return self.values[what]
            if "_set_" in name:
                self.values[what] = args[0]
            return 0
        return call


def counting_engine(**kw):
    e = E.Engine.__new__(E.Engine)
    e._L, e._h, e._owner, e.device = CountingLibrary(**kw), None, None, 0
    return e


def test_settings_set_what_differs_and_restore_it_in_reverse_order():
    e = counting_engine()
    with e.settings(search="reference", arith="fast", trials=32, typical_layers=6) as inside:
        assert inside is e and (e.swd_search(), e.swd_arith(), e.swd_trials()) == ("reference", "fast", 32)
        inner = len(e._L.calls)
    S, A, T = "set_swd_search", "set_swd_arith", "set_swd_trials"
    assert e._L.calls[:inner - 3] == [("get_swd_search",), (S, E.SEARCH_REFERENCE), ("get_swd_arith",), ("get_swd_trials",), (T, 32),
                                      ("set_typical_layers", 6)]                  # arith equals the engine's: read, not set
    assert e._L.calls[inner:] == [("set_typical_layers", 0), (T, 0), (S, E.SEARCH_FAST)]
    assert e._L.values == dict(search=E.SEARCH_FAST, arith=E.ARITH_FAST, trials=0, typical_layers=0)
    e = counting_engine()
    with e.settings():
        pass
    with e.searching(None), e.computing(None), e.trying(None):
        pass
    assert e._L.calls == []
    with e.searching("fast"), e.computing("fast"), e.trying(0):                    # the engine's own values: read only
        pass
    assert [c[0] for c in e._L.calls] == ["get_swd_search", "get_swd_arith", "get_swd_trials"]
    e = counting_engine()
    with e.searching("fast_rayleigh"), e.computing("exact"), e.trying(64):
        assert (e.swd_search(), e.swd_arith(), e.swd_trials()) == ("fast_rayleigh", "exact", 64)
    assert (e.swd_search(), e.swd_arith(), e.swd_trials()) == ("fast", "fast", 0)
    assert [c for c in e._L.calls if c[0].startswith("set_")][3:] == [(T, 0), (A, E.ARITH_FAST), (S, E.SEARCH_FAST)]


def test_settings_restore_when_the_body_or_a_setter_raises():
    e = counting_engine()
    with pytest.raises(KeyError):
        with e.settings(search="reference", arith="exact", trials=32, typical_layers=4):
            raise KeyError("body")
    assert e._L.values == dict(search=E.SEARCH_FAST, arith=E.ARITH_FAST, trials=0, typical_layers=0)
    assert [c[0] for c in e._L.calls[-4:]] == ["set_typical_layers", "set_swd_trials", "set_swd_arith", "set_swd_search"]
    with pytest.raises(ValueError, match="arith must be"):
        with e.settings(search="reference", arith="quick"):
            raise AssertionError("not reached")
    assert e._L.values["search"] == E.SEARCH_FAST                                  # what was set before the refusal is restored


def window_calls(search, arith, engine_trials=0, fail=False):
    """the library calls of one DeviceChains.iterate() around its evaluate call, on a counting library: a DeviceChains with what
    iterate() reads and an engine whose chain and evaluate entries do nothing"""
    e = counting_engine(trials=engine_trials)
    buf = types.SimpleNamespace(data_ptr=lambda: 0)                                # (iterate() passes addresses on, nothing reads them)

    def evaluate(*args):
        if fail:
            raise RuntimeError("evaluate")
    e.chain_propose_window = e.chain_accept_window = lambda *a, **k: None
    e.evaluate_batch_dev = evaluate
    dc = DeviceChains.__new__(DeviceChains)
    dc.engine, dc.search, dc.arith, dc.C, dc.depth, dc.ld, dc.ML = e, search, arith, 8, 3, 56, 11
    dc.iiter, dc.iter_phase1, dc.iter_phase2, dc.thinning, dc.swap_every, dc.snap_in_run = 1, 40, 40, 1, 0, False
    dc.launches, dc._hint, dc._rec, dc.absent, dc.prior_records, dc.sites, dc.cfg, dc.state = 1, 5, None, None, None, None, None, None
    dc.t = dict({k: buf for k in ("lay_n", "lay_h", "lay_vp", "lay_vs", "lay_rho", "pnoise")}, beta=None)
    dc.logL = dc.mis = dc.err = buf
    if fail:
        with pytest.raises(RuntimeError, match="evaluate"):
            dc.iterate()
    else:
        assert dc.iterate() == 3 and dc.iiter == 4
    assert e._L.values == dict(search=E.SEARCH_FAST, arith=E.ARITH_FAST, trials=engine_trials, typical_layers=0)
    return len(e._L.calls)


def test_library_calls_per_window():
    """the four cases of profiles/device_chains_refactor.txt, with its counts: the parent's iterate() makes 7 / 11 / 5 / 11"""
    assert window_calls("fast", "fast") == 7                   # equal to the engine's
    assert window_calls("reference", "exact") == 11            # different from it
    assert window_calls(None, None) == 5                       # None: whatever the engine is set to
    assert window_calls("reference", "exact", fail=True) == 11  # a raising body restores all four
    assert window_calls("fast", "fast", engine_trials=32) == 5  # (the parent: 7 -- it set the trials whatever they were)


# ---- what other modules import --------------------------------------------------------------------------------------------------------

def test_names_and_methods_are_where_they_were():
    for name in ("DeviceChains", "LADDER_ADAPT_DEFAULTS", "SHARED_INITPARAMS", "SITE_INITPARAMS", "auto_spec_depth", "ladder_adapt_options",
                 "record_rows", "set_station_fields", "site_dicts", "snapshot_count", "window_entries", "RECORD_MODES"):
        assert hasattr(DC, name), name
    public = ["HINT_EVERY", "TRIALS", "diagnostics", "exchange", "iterate", "ladder_diagnostics", "ladder_evidence", "ladder_swaps", "nsamples",
              "nswaps", "posterior_classes", "posterior_covariance", "posterior_datafits", "posterior_features", "posterior_hist2d",
              "posterior_models", "posterior_moho", "posterior_residuals", "posterior_scalars", "run", "samples", "samples_dev", "save",
              "state_host", "window"]
    assert sorted(n for n in dir(DeviceChains) if not n.startswith("_")) == sorted(public)
    for private in ("_allocate_store", "_cold_mask", "_host_rows", "_save_sites", "_site_block", "_snapshot", "_store_range", "_store_rows"):
        assert callable(getattr(DeviceChains, private)), private
    from bayhunter_amd.device_chains_store import ChainStore
    assert issubclass(DeviceChains, ChainStore) and DeviceChains.samples_dev is ChainStore.samples_dev
    assert DeviceChains.__doc__.startswith("`nchains` chains on THIS rank.") and DeviceChains.__init__.__doc__ is None
