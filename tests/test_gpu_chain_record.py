"""The device record of the chains' thinned samples on the MI355X (include/bh_engine_chain_record.h, DeviceChains(record="device")).
The yardsticks are tests/chain_ref.py for the kernel and the host record (record="host": run()'s synchronise-and-copy snapshots)
for the runs -- never the record build itself.  Every comparison is for equality.

  (a) the two record builds of the window accept kernel, called directly over the crafted populations of
      tests/test_gpu_chain_kernels.py: the rows a snapshot rule worked out here from chain_ref's decisions, bit for bit; every
      other row untouched; the committed state chain_ref's (hence the non-record entry's); the refusals
  (b) run(): record="device" against record="host" -- samples of both phases, the chains' state, the saved files, fewer launches
  (c) a tempered run (cold samples) and a SiteTargets run with priors per site (the priors record build), device against host
  (d) posterior_models fed from samples_dev() against the same call on the host arrays

Two statements of the issue this file cannot take literally, and what it asserts instead:
  * "at least one row from a node >= 64": a row holds the state BEFORE a level is decided, so its source is a node of an earlier
    level; in the deepest window (7) the last level before which a row can be due is 6 and its sources are nodes of levels <= 5,
    i.e. nodes <= 62.  Nodes >= 64 are last-level nodes: they reach the committed state (check_states covers them, the
    all-accepted chains of depth 7) but no row of their own window.  Asserted: sources on the deepest level that can be one
    (nodes 31..62) at depth 7, sources among the pre-window state and nodes at every depth > 1.
  * "a window that starts before 0 and ends after it": iteration 0 adapts the proposal widths and must be the last of its window,
    so the furthest such a window reaches is 0 itself; that window (iiter = 1 - depth) is added to the populations here.
  * state_host() "array for array": the chains' state, every array (STATE and beta); the proposal and layer arrays are the
    workspace of the LAST window, which is cut differently by design -- they are compared at spec_depth 1, where the windows of
    both runs are the same.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import chain_ref as R
from conftest import golden
import bayhunter_amd as bh
from bayhunter_amd import engine as E
from bayhunter_amd.device_chains import DeviceChains, record_rows, snapshot_count
from bayhunter_amd.posterior import posterior_models
from test_gpu_chain_kernels import Device, make_cfg, table, run_propose, check_states, STATE
from test_gpu_chains import SETUPS, make_targets
from test_gpu_sites_priors import SITE_INIT, SITE_PRIORS, full_site

pytestmark = pytest.mark.gpu

FILL = -7777.0                         # no kernel writes it: states, logL and misfits of the populations are nowhere near
ARRAYS = ("models", "likes", "vpvs", "misfits", "noise")


class Store(object):
    """a bh_chain_record over torch tensors, every element FILL"""

    def __init__(self, dv, rows, thinning, row0, beta):
        torch = dv.torch
        dev = torch.device("cuda", 0)
        C, ML, nt = dv.C, dv.ML, dv.nt
        shapes = dict(models=(rows, C, 2 * ML), likes=(rows, C), vpvs=(rows, C), misfits=(rows, C, nt + 1), noise=(rows, C, 2 * nt))
        self.t = {k: torch.full(sh, FILL, dtype=torch.float32, device=dev) for k, sh in shapes.items()}
        self.t["beta"] = torch.full((rows, C), FILL, dtype=torch.float64, device=dev) if beta else None
        torch.cuda.synchronize(dev)
        self.rec = E.ChainRecord()
        for k, v in self.t.items():
            setattr(self.rec, k, None if v is None else v.data_ptr())
        self.rec.rows, self.rec.thinning, self.rec.row0 = rows, thinning, row0
        self.eng = dv.eng

    def host(self):
        self.eng.synchronize()
        return {k: v.cpu().numpy() for k, v in self.t.items() if v is not None}


def untouched(a):
    return bool(np.all(a == a.dtype.type(FILL)))


@functools.lru_cache(maxsize=None)
def reference(C, ML, nt, depth):
    """chain_ref's trees, synthetic likelihoods and walks of the populations, made once and shared by every thinning (read only)"""
    pops = list(R.accept_populations(C, ML, nt, depth))
    pops.append(("plain", R.population("plain", C, ML, nt, depth, 1 - depth, seed=4), False))     # ... -1, 0: ends at the adaptation of 0
    out = []
    for build, pop, beta in pops:
        tr = R.trees(pop)
        ap = R.accept_population(pop, tr, beta=beta)
        out.append((build, pop, beta, tr, ap, R.walk(pop, tr, ap)))
    return out


def expected_row(pop, tr, ap, res, c, k):
    """chain c's state before level k of the window is decided, as the store holds it -> (dict of float32 arrays, source):
    source -1 = the pre-window state, else the node accepted last at a level < k (chain_ref's decisions)"""
    ML, nt = pop["ML"], pop["nt"]
    src = -1
    for d in res[c][1]:
        if d["k"] < k and d["accepted"]:
            src = d["node"]
    if src < 0:
        s = ap["states"][c]
        like, mis = s["like"], s["misfits"]
    else:
        s = tr[c]["nodes"][src]
        like, mis = ap["logL"][src, c], ap["misfits"][src, c]
    n = int(s["n"])
    row = np.full(2 * ML, np.nan, dtype=np.float32)
    row[:n], row[n:2 * n] = np.asarray(s["vs"], dtype=np.float64).astype(np.float32), np.asarray(s["z"], dtype=np.float64).astype(np.float32)
    return dict(models=row, likes=np.float32(np.float64(like)), vpvs=np.float32(np.float64(s["vpvs"])),
                misfits=np.asarray(mis, dtype=np.float64).astype(np.float32), noise=np.asarray(s["noise"], dtype=np.float64).astype(np.float32)), src


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def accept_record(engine, dv, build, pop, ap, store):
    """one launch of the record entry of `build`; -> what must stay alive until the engine's stream is waited for"""
    C, ML, depth = dv.C, dv.ML, dv.depth
    logL, mis = dv.upload(dv.columns(ap["logL"])), dv.upload(dv.columns(ap["misfits"]))
    if build == "plain":
        engine.chain_accept_window_record(make_cfg(pop["priors"][0], ML), dv.state, C, pop["iiter"], depth, dv.ld, logL.data_ptr(),
                                          mis.data_ptr(), store.rec)
        return logL, mis
    tab, po = table(dv, pop["recs"]), dv.upload(pop["prior_of"], np.int32)
    engine.chain_accept_window_priors_record(make_cfg(pop["priors"][0], ML, own=False), dv.state, C, pop["iiter"], depth, dv.ld,
                                             logL.data_ptr(), mis.data_ptr(), tab.data_ptr(), len(pop["recs"]), po.data_ptr(), store.rec)
    return logL, mis, tab, po


@pytest.mark.parametrize("depth", [1, 3, 7])
@pytest.mark.parametrize("C,ML,nt", [(37, 4, 1), (70, 32, 8)])
def test_record_builds_write_the_rows_of_the_reference_walk(engine, C, ML, nt, depth):
    """(a) Plain and priors record builds, beta NULL and set, thinning 1, 2 and 3, windows that end at 1000, -1000 and 0 and one
    without adaptation; depth 1 runs the window kernel too (wide ld or not: the record entries have no lane kernel).  (70, 32, 8) is
    the header's limit: a model row of exactly 64 floats.  Chains whose record index is out of range keep their state, and that state
    is what their rows hold."""
    wide = depth != 3
    sources = set()
    for thinning in (1, 2, 3):
        for build, pop, beta, tr, ap, res in reference(C, ML, nt, depth):
            iiter = pop["iiter"]
            due = [k for k in range(depth) if (iiter + k) % thinning == 0]          # Python's %: the non-negative residue
            assert len(due) == snapshot_count(iiter, iiter + depth, thinning)
            row0, spare = 2, 3
            rows = row0 + len(due) + spare
            dv = Device(engine, ap["states"], ML, nt, depth, wide, ap["draws"], beta=ap["beta"])
            run_propose(engine, dv, build, dict(pop, states=ap["states"], draws=ap["draws"]))
            store = Store(dv, rows, thinning, row0, beta)
            keep = accept_record(engine, dv, build, pop, ap, store)
            got = store.host()
            del keep
            what = (build, iiter, beta, thinning)
            for j, k in enumerate(due):
                for c in range(C):
                    exp, src = expected_row(pop, tr, ap, res, c, k)
                    sources.add(src)
                    for name in ARRAYS:
                        assert same_bits(got[name][row0 + j, c], exp[name]), what + (k, c, src, name, got[name][row0 + j, c], exp[name])
                    if beta:
                        assert got["beta"][row0 + j, c] == ap["beta"][c], what + (k, c)
            for name, a in got.items():                                   # nothing but the due rows was written
                assert untouched(a[:row0]) and untouched(a[row0 + len(due):]), what + (name,)
            assert (beta and "beta" in got) or (not beta and "beta" not in got)
            check_states(dv, res, what)                                   # the committed state is the reference's
    assert -1 in sources
    if depth > 1:
        assert any(0 <= s < 31 for s in sources), sorted(sources)
    if depth == 7:
        assert any(31 <= s < 63 for s in sources), sorted(sources)      # the deepest level a row's source can lie on
    assert all(s < (1 << (depth - 1)) - 1 for s in sources)              # ... never a node of the window's last level


def test_record_entries_refuse_what_the_header_says(engine):
    """BH_EINVAL, nothing launched: the store keeps its fill everywhere and the chains their state"""
    C, ML, nt, depth = 37, 4, 1, 3
    build, pop, beta, tr, ap, res = reference(C, ML, nt, depth)[3]          # (priors build at LATE = 201: levels 201, 202, 203)
    assert build == "priors" and pop["iiter"] == R.LATE
    dv = Device(engine, ap["states"], ML, nt, depth, False, ap["draws"], beta=ap["beta"])
    run_propose(engine, dv, build, dict(pop, states=ap["states"], draws=ap["draws"]))
    before = dv.host(STATE)
    logL, mis = dv.upload(dv.columns(ap["logL"])), dv.upload(dv.columns(ap["misfits"]))
    tab, po = table(dv, pop["recs"]), dv.upload(pop["prior_of"], np.int32)
    L = engine._L
    cfg_p, cfg_o = make_cfg(pop["priors"][0], ML), make_cfg(pop["priors"][0], ML, own=False)

    def call(store, rec, iiter=pop["iiter"]):
        a = (engine.stream, ctypes.byref(cfg_p), ctypes.byref(dv.state), C, iiter, depth, dv.ld, logL.data_ptr(), mis.data_ptr())
        b = (engine.stream, ctypes.byref(cfg_o), ctypes.byref(dv.state), C, iiter, depth, dv.ld, logL.data_ptr(), mis.data_ptr(),
             tab.data_ptr(), len(pop["recs"]), po.data_ptr())
        return L.bh_chain_accept_window_record(*a, rec), L.bh_chain_accept_window_priors_record(*b, rec)

    store = Store(dv, 4, 2, 0, False)
    m = snapshot_count(pop["iiter"], pop["iiter"] + depth, 2)
    assert m == 1                                                            # (202)
    cases = []
    store.rec.row0 = store.rec.rows - m + 1                                  # row0 + m = rows + 1
    cases.append(("one row too many", call(store, ctypes.byref(store.rec))))
    store.rec.row0 = 0
    store.rec.thinning = 0
    cases.append(("thinning 0", call(store, ctypes.byref(store.rec))))
    store.rec.thinning = 2
    store.rec.models = None
    cases.append(("models NULL", call(store, ctypes.byref(store.rec))))
    store.rec.models = store.t["models"].data_ptr()
    store.rec.row0 = -1
    cases.append(("row0 < 0", call(store, ctypes.byref(store.rec))))
    store.rec.row0 = 0
    cases.append(("rec NULL", call(store, None)))
    cases.append(("adaptation inside the window", call(store, ctypes.byref(store.rec), iiter=999)))
    for name, rcs in cases:
        assert rcs == (E.BH_EINVAL, E.BH_EINVAL), (name, rcs)
    got = store.host()
    assert all(untouched(a) for a in got.values())
    after = dv.host(STATE)
    for k in STATE:
        assert after[k].tobytes() == before[k].tobytes(), k
    # ... and the last row of the store is a row like any other: row0 + m = rows is accepted (the priors entry, then its rows checked)
    store.rec.row0 = store.rec.rows - m
    rc = L.bh_chain_accept_window_priors_record(engine.stream, ctypes.byref(cfg_o), ctypes.byref(dv.state), C, pop["iiter"], depth, dv.ld,
                                                logL.data_ptr(), mis.data_ptr(), tab.data_ptr(), len(pop["recs"]), po.data_ptr(),
                                                ctypes.byref(store.rec))
    assert rc == E.BH_OK
    got = store.host()
    for c in range(C):
        exp, _ = expected_row(pop, tr, ap, res, c, 1)
        for name in ARRAYS:
            assert same_bits(got[name][3, c], exp[name]), (c, name)
    assert all(untouched(a[:3]) for a in got.values())
    check_states(dv, res, ("last row",))


# ---- runs: record="device" against record="host" ---------------------------------------------------------------------------
CHAIN_STATE = STATE + ("beta",)


def same_dict(a, b, what):
    assert sorted(a) == sorted(b), (what, sorted(a), sorted(b))
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
            continue
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k, x.dtype, y.dtype, x.shape, y.shape)
        assert np.array_equal(x, y, equal_nan=(x.dtype.kind == "f")), (what, k)


def same_files(pa, pb):
    files = sorted(f for f in os.listdir(pa) if f.endswith(".npy"))
    assert files and files == sorted(f for f in os.listdir(pb) if f.endswith(".npy"))
    for f in files:
        x, y = np.load(os.path.join(pa, f)), np.load(os.path.join(pb, f))
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=True), f
    return files


@pytest.mark.parametrize("depth", [1, 3, 7])
@pytest.mark.parametrize("maxmodels,thinning", [(250, 1), (36, 7)])
def test_a_run_records_on_the_device_what_it_records_on_the_host(tmp_path, maxmodels, thinning, depth):
    """(b) The set-up of test_speculative_windows_walk_the_sequential_trajectory with 5 chains: 1150 + 250 iterations across the
    adaptations at -1000 and 0; thinning 1 (every iteration kept) and 7 (the burn-in no multiple of it)."""
    g = golden("chain_golden.npz")
    su = SETUPS["exp"]
    runs = {}
    for record in ("host", "device"):
        init = dict(su["init"], iter_burnin=1150, iter_main=250, maxmodels=maxmodels, savepath=str(tmp_path / record))
        runs[record] = DeviceChains(make_targets(g), 5, init, su["priors"], seed=20260928, spec_depth=depth, record=record).run()
    host, dev = runs["host"], runs["device"]
    assert host.thinning == dev.thinning == thinning and dev.iiter == host.iiter == 250
    r1, r2 = record_rows(1150, 250, thinning)
    for phase, rows in (("p1", r1), ("p2", r2)):
        a, b = host.samples(phase), dev.samples(phase)
        assert a["models"].shape == (rows, 5, 2 * host.ML) and dev.nsamples(phase) == host.nsamples(phase) == rows
        same_dict(a, b, (phase,))
    sa, sb = host.state_host(), dev.state_host()
    same_dict({k: sa[k] for k in CHAIN_STATE}, {k: sb[k] for k in CHAIN_STATE}, ("state",))
    if depth == 1:                                  # the same windows: the workspace of the last one as well
        same_dict(sa, sb, ("state and workspace",))
    files = same_files(host.save(), dev.save())
    assert len(files) == 5 * 2 * 5
    if thinning == 1:
        assert host.launches == 1400                # one per iteration, each behind a synchronisation
        if depth == 7:
            assert dev.launches < host.launches and dev.launches < 1400 / 4
    assert not dev.snap["p1"] and not dev.snap["p2"]


@pytest.fixture(scope="module")
def site_runs(tmp_path_factory):
    """2 sites x 4 chains under their own priors (sites 0 and 1 of tests/test_gpu_sites_priors.py), host and device record"""
    g = golden("chain_golden.npz")
    root = tmp_path_factory.mktemp("record_sites")
    out = {}
    for record in ("host", "device"):
        st = bh.SiteTargets([full_site(g, s, "phase_rf") for s in range(2)], names=["st0", "st1"], per_site_x="all", per_site_rf=True)
        inits = [dict(SITE_INIT[s], savepath=str(root / record)) for s in range(2)]
        out[record] = DeviceChains(st, 4, inits, SITE_PRIORS[:2], seed=77, search="fast", record=record).run()
    return out


def test_sites_with_their_own_priors_record_on_the_device(site_runs):
    """(c) the priors record build in a run: samples(site=s) of both sites and both phases, and the saved folders"""
    host, dev = site_runs["host"], site_runs["device"]
    assert dev.prior_table and dev.depth > 1 and dev.thinning == 5 and dev.launches < host.launches
    for s in range(2):
        for phase in ("p1", "p2"):
            a, b = host.samples(phase, site=s), dev.samples(phase, site=s)
            assert a["models"].shape[-1] == 2 * (SITE_PRIORS[s]["layers"][1] + 1) and a["models"].shape[0] > 0
            same_dict(a, b, (s, phase))
    same_dict(host.samples("p2"), dev.samples("p2"), ("all",))
    sa, sb = host.state_host(), dev.state_host()
    same_dict({k: sa[k] for k in CHAIN_STATE}, {k: sb[k] for k in CHAIN_STATE}, ("state",))
    for pa, pb in zip(host.save(), dev.save()):
        same_files(pa, pb)


def test_a_tempered_run_records_on_the_device():
    """(c) two ladders of 4 temperatures, exchanges every 20 iterations, thinning 4: every fifth snapshot falls on an exchange
    iteration and must show the temperatures AFTER the exchange, as the host snapshot does"""
    g = golden("chain_golden.npz")
    su = SETUPS["exp"]
    init = dict(su["init"], iter_burnin=280, iter_main=60, maxmodels=15)
    ladder = np.repeat(np.arange(2), 4)
    betas = np.tile(1.0 / np.geomspace(1.0, 20.0, 4), 2)
    runs = {}
    for record in ("host", "device"):
        runs[record] = DeviceChains(make_targets(g), 8, init, su["priors"], seed=5, betas=betas, ladder=ladder, swap_every=20,
                                    record=record).run()
    host, dev = runs["host"], runs["device"]
    assert host.thinning == 4 and host.nswaps == dev.nswaps and host.nswaps > 0 and dev.launches < host.launches
    for phase in ("p1", "p2"):
        a = host.samples(phase)
        assert a["beta"].dtype == np.float64 and (phase == "p2" or not np.array_equal(a["beta"][0], a["beta"][-1]))   # (they moved)
        same_dict(a, dev.samples(phase), (phase,))
        c = host.samples(phase, cold_only=True)
        assert c["models"].shape[1] == 2 and np.all(c["beta"] == 1.0)
        same_dict(c, dev.samples(phase, cold_only=True), (phase, "cold"))
    sa, sb = host.state_host(), dev.state_host()
    same_dict({k: sa[k] for k in CHAIN_STATE}, {k: sb[k] for k in CHAIN_STATE}, ("state",))


def test_posterior_models_from_the_device_store(site_runs):
    """(d) samples_dev() hands views of the store to the posterior kernels: the summaries of both sites equal those of the same
    call on the host record's arrays"""
    import torch
    host, dev = site_runs["host"], site_runs["device"]
    d = dev.samples_dev("p2")
    h = host.samples("p2")
    rows, C = h["models"].shape[:2]
    assert d["models"].shape == h["models"].shape and d["models"].is_cuda and d["models2d"].shape == (rows * C, 2 * dev.ML)
    assert d["models2d"].data_ptr() == d["models"].data_ptr() == dev.store["models"].data_ptr() + 4 * dev._store_range("p2")[0] * C * 2 * dev.ML
    assert d["site"].dtype == torch.int32 and np.array_equal(d["site"].cpu().numpy(), np.tile(np.arange(C) // 4, rows))
    for k in ARRAYS:
        assert np.array_equal(d[k].cpu().numpy(), h[k], equal_nan=True), k
    assert "beta" not in d
    a = posterior_models(d["models2d"], site=d["site"], nsites=2)
    b = posterior_models(h["models"].reshape(rows * C, -1), site=np.tile(np.arange(C) // 4, rows).astype(np.int32), nsites=2)
    assert len(a) == len(b) == 2
    for s in range(2):
        assert sorted(a[s]) == sorted(b[s]) and a[s]["count"] == b[s]["count"] > 0
        for k in a[s]:
            if isinstance(a[s][k], tuple):
                for x, y in zip(a[s][k], b[s][k]):
                    assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True), (s, k)
            else:
                assert a[s][k] == b[s][k], (s, k)
    with pytest.raises(E.EngineError):
        host.samples_dev()
