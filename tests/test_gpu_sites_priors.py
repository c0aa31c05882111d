"""Sites that carry their own priors and sampler settings, on the MI355X (include/bh_engine_sites_priors.h, DeviceChains with a
sequence of dicts).  The rule under test: every site of such a run walks the chains of its one-site DeviceChains made with the
site's own dicts, bit for bit.  The one-site run goes through the kernels without a table: it is the reference here, not the
code under test.  Runs are made once per (structure, search, depth) and shared by the tests that look at them."""
import os

import numpy as np
import pytest

from conftest import golden
import bayhunter_amd as bh
from bayhunter_amd import engine as E
from bayhunter_amd.device_chains import DeviceChains
from test_gpu_sites_x import PRIORS, _RefUnpickler
from test_gpu_sites_missing import chain_slots, own_targets, same_samples, CHAIN_KP, CHAIN_KL, CHAIN_KG, CHAIN_P

pytestmark = pytest.mark.gpu

S, C, SEED = 4, 3, 77       # three chains per site: site boundaries fall inside a wavefront of the window propose kernel
INIT = dict(nchains=1, iter_burnin=150, iter_main=75, acceptance=(40, 80), thickmin=0.1, lvz=0.1, hvz=None, rcond=None, maxmodels=15)
# Together the sites differ in every field of a record.  Sites 0 and 3 differ in the acceptance band only.
SITE_PRIORS = [
    dict(PRIORS, layers=(1, 20)),
    dict(PRIORS, layers=(1, 8), vs=(2.5, 4.5), z=(0, 50), mohoest=(35, 3), rfnoise_sigma=(1e-4, 0.03), swdnoise_sigma=(1e-4, 0.05)),
    dict(PRIORS, layers=(2, 20), vpvs=1.73, mantle=(4.2, 1.8), rfnoise_sigma=0.01, swdnoise_sigma=0.03),
    dict(PRIORS, layers=(1, 20)),
]
SITE_INIT = [
    dict(INIT),
    dict(INIT, thickmin=0.3, lvz=None, hvz=0.5, propdist=(0.02, 0.03, 0.02, 0.004, 0.006), acceptance=(30, 60)),
    dict(INIT, lvz=0.2),
    dict(INIT, acceptance=(10, 20)),
]
NARROW, FIXED = 1, 2        # the site with the narrower ranges and the smaller capacity; the site with fixed vp/vs and sigmas
KINDS = {"phase_rf": ("rph", "lph", "prf"), "group": ("rph", "rgr", "prf")}


def full_site(g, s, name):
    """site s with every target of the structure (the data of tests/test_gpu_sites_missing.py's sites)"""
    rs = np.random.RandomState(500 + s)
    xs, ys = np.asarray(g["xsw"], dtype=float), np.asarray(g["ysw"], dtype=float)
    made = {}
    x1 = np.linspace(xs.min() + 0.3 * s, xs.max() - 1.1 * s, CHAIN_KP[s])
    made["rph"] = bh.RayleighDispersionPhase(x1, np.interp(x1, xs, ys) + rs.normal(0, 0.02, x1.size))
    x2 = np.linspace(xs.min() + 0.5 * s, xs.max() - 0.2 * s, CHAIN_KL[s])
    made["lph"] = bh.LoveDispersionPhase(x2, 1.05 * np.interp(x2, xs, ys) + rs.normal(0, 0.02, x2.size))
    x3 = np.linspace(xs.min() + 0.7 * s, xs.max() - 0.4 * s, CHAIN_KG[s])
    made["rgr"] = bh.RayleighDispersionGroup(x3, 0.9 * np.interp(x3, xs, ys) + rs.normal(0, 0.02, x3.size))
    t = bh.PReceiverFunction(g["xrf"], g["yrf"] + rs.normal(0, 0.01, g["yrf"].size))
    t.moddata.plugin.set_modelparams(gauss=1.0, p=CHAIN_P[s])
    made["prf"] = t
    return bh.JointTarget([made[k] for k in KINDS[name]])


def site_inits(root, kind):
    return [dict(ip, savepath=str(root / kind)) for ip in SITE_INIT]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """get(name, search, depth) -> (the four-site run, its four one-site runs, the folder they save below), made once"""
    g = golden("chain_golden.npz")
    made = {}

    def get(name, search, depth):
        key = (name, search, depth)
        if key not in made:
            root = tmp_path_factory.mktemp("priors")
            names = ["st%d" % s for s in range(S)]
            st = bh.SiteTargets([full_site(g, s, name) for s in range(S)], names=names, per_site_x="all", per_site_rf=True)
            dc = DeviceChains(st, C, site_inits(root, "multi"), SITE_PRIORS, seed=SEED, spec_depth=depth, search=search).run()
            assert dc.prior_table and (dc.depth > 1 or depth == 1)
            ones = []
            for s in range(S):
                ip = dict(SITE_INIT[s], savepath=str(root / "one" / names[s]), station=names[s])
                ones.append(DeviceChains(full_site(g, s, name), C, ip, SITE_PRIORS[s], seed=SEED, chain_offset=s * C, spec_depth=depth,
                                         search=search).run())
                assert not ones[-1].prior_table
            made[key] = (dc, ones, root)
        return made[key]
    return get


def same_state(dc, one, s, what):
    a, b = dc.state_host(), one.state_host()
    for k in ("proposed", "accepted", "propdist"):
        assert np.array_equal(a[k][:, s * C:(s + 1) * C], b[k]), "%s: %s" % (what, k)


@pytest.mark.parametrize("depth", [None, 1, 3])
@pytest.mark.parametrize("name,search", [("phase_rf", "fast"), ("group", "reference")])
def test_every_site_walks_its_one_site_run(runs, name, search, depth):
    dc, ones, root = runs(name, search, depth)
    assert dc.ML == 21 and dc.site_ML == [21, 9, 21, 21]
    for s in range(S):
        what = "%s %s depth %s site %d" % (name, search, depth, s)
        for phase in ("p1", "p2"):
            a = dc.samples(phase, site=s)
            assert a["models"].shape[-1] == 2 * (SITE_PRIORS[s]["layers"][1] + 1)       # the site's own row width
            same_samples(a, ones[s].samples(phase), what + " " + phase)
        same_state(dc, ones[s], s, what)
    assert dc.samples("p2")["models"].shape[-1] == 2 * 21                              # all chains: the shared width
    if depth is not None:
        return
    paths = dc.save()                   # the saved folder of a site is that of its one-site run
    for s in range(S):
        dpath = ones[s].save()
        files = sorted(f for f in os.listdir(dpath) if f.endswith(".npy"))
        assert files and files == sorted(f for f in os.listdir(paths[s]) if f.endswith(".npy"))
        for f in files:
            assert np.array_equal(np.load(os.path.join(dpath, f)), np.load(os.path.join(paths[s], f)), equal_nan=True), f
        with open(os.path.join(paths[s], "st%d_config.pkl" % s), "rb") as f:
            cfg = _RefUnpickler(f).load()
        assert cfg["priors"] == dict(bh.chains.DEFAULT_PRIORS, **SITE_PRIORS[s])
        for k in ("acceptance", "thickmin", "lvz", "hvz"):
            assert cfg["initparams"][k] == SITE_INIT[s][k]
        assert cfg["initparams"]["station"] == "st%d" % s


def interfaces(models, ML):
    """[rows, ML] nuclei -> (vs, interface depths) as flat arrays over every sampled model"""
    vs_all, zi_all = [], []
    for row in models.reshape(-1, 2 * ML):
        n = int(np.isfinite(row).sum()) // 2
        vs, z = row[:n].astype(np.float64), row[n:2 * n].astype(np.float64)
        vs_all.append(vs)
        zi_all.append((z[:-1] + z[1:]) / 2.)
    return np.concatenate(vs_all), np.concatenate(zi_all)


@pytest.mark.parametrize("name,search", [("phase_rf", "fast"), ("group", "reference")])
def test_the_settings_took_effect(runs, name, search):
    dc, ones, _ = runs(name, search, None)
    st = dc.state_host()
    blk = lambda s: slice(s * C, (s + 1) * C)
    for s in range(S):      # vp/vs moves (PAR_MAP: index 4) at every site but the one that fixes vp/vs
        assert np.all(st["proposed"][4, blk(s)] == 0) if s == FIXED else np.all(st["proposed"][4, blk(s)] > 0), s
    inside = {}
    for s in range(S):
        pr = SITE_PRIORS[s]
        ML = pr["layers"][1] + 1
        for phase in ("p1", "p2"):
            smp = dc.samples(phase, site=s)
            vs, zi = interfaces(smp["models"], ML)
            # (float32 rounding is monotonic: a value inside the range in double is inside the rounded range)
            assert vs.min() >= np.float32(pr["vs"][0]) and vs.max() <= np.float32(pr["vs"][1]), (s, vs.min(), vs.max())
            if zi.size:     # interface depths are formed here from the float32 nuclei: a float32 ulp of 60 km
                assert zi.min() >= pr["z"][0] - 1e-5 and zi.max() <= pr["z"][1] + 1e-5, (s, zi.min(), zi.max())
            nlay = np.isfinite(smp["models"]).sum(axis=-1) // 2 - 1
            assert nlay.min() >= pr["layers"][0] and nlay.max() <= pr["layers"][1]
            sig = smp["noise"][..., 1::2]
            if s == FIXED:      # fixed sigmas stay what they are; vp/vs too
                assert np.all(sig[..., :2] == np.float32(pr["swdnoise_sigma"])) and np.all(sig[..., 2] == np.float32(pr["rfnoise_sigma"]))
                assert np.all(smp["vpvs"] == np.float32(pr["vpvs"]))
            else:
                assert np.unique(sig[..., 0]).size > 1 and np.unique(smp["vpvs"]).size > 1
                for j, key in enumerate(("swdnoise_sigma", "swdnoise_sigma", "rfnoise_sigma")):
                    assert sig[..., j].min() >= np.float32(pr[key][0]) and sig[..., j].max() <= np.float32(pr[key][1]), (s, key)
            if phase == "p2":
                lo, hi = SITE_PRIORS[NARROW]["vs"]
                inside[s] = bool(vs.min() >= np.float32(lo) and vs.max() <= np.float32(hi))
    assert inside[NARROW] and not all(inside[s] for s in range(S) if s != NARROW)
    # sites 0 and 3 differ in their acceptance band only, and start from the same widths: the adaptation ran
    assert SITE_PRIORS[0] == SITE_PRIORS[3] and {k for k in SITE_INIT[0] if SITE_INIT[0][k] != SITE_INIT[3][k]} == {"acceptance"}
    assert not np.array_equal(st["propdist"][:, blk(0)], st["propdist"][:, blk(3)])
    start = np.asarray(bh.chains.DEFAULT_INITPARAMS["propdist"])[:, None]
    assert np.any(st["propdist"][:, blk(0)] != start) and np.any(st["propdist"][:, blk(3)] != start)


@pytest.mark.parametrize("depth", [None, 1])
def test_together_with_missing_targets(depth, tmp_path):
    """missing=True with the "phase_rf" structure of tests/test_gpu_sites_missing.py and noise priors per site: every site
    equals its one-site run over the targets it has, noise and misfits in the site's own columns"""
    g = golden("chain_golden.npz")
    name = "phase_rf"
    st = bh.SiteTargets([chain_slots(g, s, name) for s in range(S)], per_site_x="all", per_site_rf=True, missing=True)
    dc = DeviceChains(st, C, site_inits(tmp_path, "multi"), SITE_PRIORS, seed=SEED, spec_depth=depth).run()
    assert dc.prior_table and dc.absent is not None
    for s in range(S):
        one = DeviceChains(own_targets(g, s, name), C, SITE_INIT[s], SITE_PRIORS[s], seed=SEED, chain_offset=s * C, spec_depth=depth).run()
        k = int(st.present[s].sum())
        for phase in ("p1", "p2"):
            a = dc.samples(phase, site=s)
            assert a["noise"].shape[-1] == 2 * k and a["misfits"].shape[-1] == k + 1
            same_samples(a, one.samples(phase), "missing site %d %s" % (s, phase))
        same_state(dc, one, s, "missing site %d" % s)
    assert (~st.present).any(axis=1).sum() == 3


@pytest.mark.parametrize("depth", [None, 1])
def test_the_table_with_equal_priors_gives_the_bits_of_the_run_without_it(depth):
    g = golden("chain_golden.npz")
    mk = lambda: bh.SiteTargets([full_site(g, s, "phase_rf") for s in range(S)], per_site_x="all", per_site_rf=True)
    a = DeviceChains(mk(), C, INIT, PRIORS, seed=SEED, spec_depth=depth).run()
    b = DeviceChains(mk(), C, [INIT] * S, [PRIORS] * S, seed=SEED, spec_depth=depth, prior_table=True).run()
    assert not a.prior_table and a.prior_records is None and b.prior_table and b.prior_records is not None
    for phase in ("p1", "p2"):
        same_samples(a.samples(phase), b.samples(phase), phase)
    sa, sb = a.state_host(), b.state_host()
    for k in ("proposed", "accepted", "propdist", "vs", "z", "noise", "like", "naccepted"):
        assert np.array_equal(sa[k], sb[k]), k


def test_sites_still_share_every_slots_noise_law():
    """one site fixes the receiver function's correlation where the others range it: another installed law, refused where the
    sites' targets are checked, with that check's message"""
    g = golden("chain_golden.npz")
    st = bh.SiteTargets([full_site(g, s, "phase_rf") for s in range(S)], per_site_x="all", per_site_rf=True)
    priors = [dict(p) for p in SITE_PRIORS]
    priors[2]["rfnoise_corr"] = 0.5
    with pytest.raises(ValueError, match=r"site 2 \(site002\), target 2 \(prf\): noise law 'gauss', site 0's 'exp'"):
        DeviceChains(st, C, SITE_INIT, priors, seed=SEED)


def test_tempered_chains_of_sites_with_their_own_priors():
    g = golden("chain_golden.npz")
    Ct = 4
    init = [dict(ip, iter_burnin=120, iter_main=60, maxmodels=10) for ip in SITE_INIT]
    betas = np.tile([1.0, 0.8, 1.0, 0.8], S)
    ladder = np.repeat(np.arange(2 * S), 2)                 # two ladders of two rungs per site
    st = bh.SiteTargets([chain_slots(g, s, "phase_rf") for s in range(S)], per_site_x="all", per_site_rf=True, missing=True)
    dc = DeviceChains(st, Ct, init, SITE_PRIORS, seed=9, betas=betas, ladder=ladder, swap_every=5).run()
    assert dc.prior_table
    for s in range(S):
        blk = slice(s * Ct, (s + 1) * Ct)
        one = DeviceChains(own_targets(g, s, "phase_rf"), Ct, init[s], SITE_PRIORS[s], seed=9, chain_offset=s * Ct, betas=betas[blk],
                           ladder=ladder[blk], swap_every=5).run()
        same_samples(dc.samples("p2", site=s), one.samples("p2"), "tempered site %d" % s)
        same_samples(dc.samples("p2", site=s, cold_only=True), one.samples("p2", cold_only=True), "cold site %d" % s)


@pytest.mark.parametrize("depth", [1, 3])
def test_a_record_index_out_of_range_leaves_the_chain_alone(depth):
    """ABI level: prior_of outside [0, P) -- every proposal of that chain invalid, its state and counters untouched, the
    evaluation fed the model it holds; the other chains walk on as if nothing were wrong.  And the entry points' refusals."""
    import torch
    g = golden("chain_golden.npz")
    mk = lambda: bh.SiteTargets([full_site(g, s, "phase_rf") for s in range(S)], per_site_x="all", per_site_rf=True)
    init = [dict(ip, iter_burnin=40, iter_main=20) for ip in SITE_INIT]
    good = DeviceChains(mk(), C, init, SITE_PRIORS, seed=SEED, spec_depth=depth)
    wild = DeviceChains(mk(), C, init, SITE_PRIORS, seed=SEED, spec_depth=depth)
    bad = [1, 7]
    of = wild.prior_of.cpu().numpy().copy()
    of[bad[0]], of[bad[1]] = S, -1
    wild.prior_of = torch.from_numpy(of).to(wild.dev)
    before = wild.state_host()
    for dc in (good, wild):
        for _ in range(12):
            dc.iterate()
    a, b = good.state_host(), wild.state_host()
    keep = np.ones(S * C, bool)
    keep[bad] = False
    N = (1 << depth) - 1
    for k in ("n", "vs", "z", "vpvs", "noise", "like", "misfits", "propdist", "proposed", "accepted", "naccepted"):
        assert np.array_equal(a[k][..., keep], b[k][..., keep]), k          # the neighbours
        assert np.array_equal(b[k][..., bad], before[k][..., bad]), k       # untouched
    assert np.any(a["proposed"][:, bad] > 0)
    cols = (np.arange(N)[:, None] * (S * C) + np.asarray(bad)[None, :]).ravel()
    assert np.all(b["valid"][cols] == 0) and np.any(b["valid"][:N * S * C] == 1)
    for c in bad:                                                           # the evaluation saw the model the chain holds
        n = before["n"][c]
        assert np.all(b["lay_n"][np.arange(N) * S * C + c] == n)
        assert np.array_equal(b["lay_vs"][:n, c], before["vs"][:n, c])
    # refusals: a null table, a null prior_of, P < 1
    e, L = wild.engine, wild.engine._L
    args = (e.stream, E.C.byref(wild.cfg), E.C.byref(wild.state), S * C, wild.iiter, 1, wild.ld)
    tab, pof = wild.prior_records.data_ptr(), wild.prior_of.data_ptr()
    out = (wild.logL.data_ptr(), wild.mis.data_ptr())
    for pr, P, po in ((None, S, pof), (tab, S, None), (tab, 0, pof)):
        assert L.bh_chain_propose_window_priors(*args, pr, P, po, None) == E.BH_EINVAL
        assert L.bh_chain_accept_window_priors(*args, *out, pr, P, po) == E.BH_EINVAL
    e.synchronize()
