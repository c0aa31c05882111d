"""Sites that carry their own priors and sampler settings (include/bh_engine_sites_priors.h, DeviceChains with a sequence of
dicts), the parts that need no GPU: the header, the library's exports and the ctypes mirror of the record, what DeviceChains
accepts and refuses, when the table is used, and what a site's record holds."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, golden
import bayhunter_amd as bh
from bayhunter_amd import engine as E
from bayhunter_amd.chains import DEFAULT_INITPARAMS, DEFAULT_PRIORS
from bayhunter_amd.device_chains import DeviceChains, SHARED_INITPARAMS, SITE_INITPARAMS, set_station_fields, site_dicts
from bayhunter_amd.sites import SiteTargets
from test_sites_missing_host import slots_of
from test_sites_x_host import X_SETS


def header_text(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", name)).read(), flags=re.S)


def test_library_exports_the_priors_header():
    raw = open(os.path.join(REPO, "include", "bh_engine_sites_priors.h")).read()
    assert '#include "bh_engine_sites_missing.h"' in raw
    txt = header_text("bh_engine_sites_priors.h")
    decl = sorted(set(re.findall(r"\b(bh_[a-z_]+)\s*\(", txt)))
    assert decl == ["bh_chain_accept_priors", "bh_chain_accept_window_priors", "bh_chain_propose_priors", "bh_chain_propose_window_priors"]
    assert sorted(E.SITE_PRIORS_SYMBOLS) == decl
    for other in (E.EXPORTED_SYMBOLS, E.DEBUG_SYMBOLS, E.SITE_SYMBOLS, E.SITE_RF_SYMBOLS, E.SITE_X_SYMBOLS, E.SITE_X_ALL_SYMBOLS,
                  E.SITE_MISSING_SYMBOLS, E.POSTERIOR_SYMBOLS):
        assert not set(decl) & set(other)
    lib = ctypes.CDLL(E.LIB_PATH)
    for name in decl:
        assert hasattr(lib, name), "missing export %s" % name
    for hdr in ("bh_engine.h", "bh_engine_debug.h", "bh_engine_sites.h", "bh_engine_sites_rf.h", "bh_engine_sites_x.h",
                "bh_engine_sites_x_all.h", "bh_engine_sites_missing.h", "bh_engine_posterior.h"):   # declared in the new header only
        other = header_text(hdr)
        assert not any(re.search(r"\b%s\b" % name, other) for name in decl) and "bh_chain_prior" not in other, hdr
    lib.bh_abi_version.restype = ctypes.c_int
    assert lib.bh_abi_version() == 10                            # extension headers are outside the contract


def test_the_ctypes_record_mirrors_the_header_and_takes_the_station_fields_of_the_config():
    txt = header_text("bh_engine_sites_priors.h")
    body = re.search(r"typedef struct bh_chain_prior \{(.*?)\} bh_chain_prior;", txt, flags=re.S).group(1)
    fields = []
    for ctype, names in re.findall(r"\b(int32_t|double)\s+([^;]+);", body):
        for nm in names.split(","):
            nm = nm.strip()
            arr = re.match(r"(\w+)\[2 \* BH_MAX_TARGETS\]", nm)
            fields.append((arr.group(1) if arr else nm, ctype, bool(arr)))
    mirror = [(k, "int32_t" if t is ctypes.c_int32 else "double", not (t is ctypes.c_int32 or t is ctypes.c_double))
              for k, t in E.ChainPrior._fields_]
    assert fields == mirror
    assert ctypes.sizeof(E.ChainPrior) == 2 * 4 + 13 * 8 + 2 * 16 * 8
    # the record and the shared part partition bh_chain_config's fields
    cfg = [k for k, _ in E.ChainConfig._fields_]
    shared = ["nt", "maxlayers", "iter_burnin", "iterations", "seed", "chain_offset"]
    assert sorted(cfg) == sorted(shared + [k for k, _, _ in fields])
    for (k, t) in E.ChainPrior._fields_:
        assert dict(E.ChainConfig._fields_)[k] is t or ctypes.sizeof(dict(E.ChainConfig._fields_)[k]) == ctypes.sizeof(t)


def two_sites(g):
    return SiteTargets([slots_of(g, X_SETS[0]), slots_of(g, X_SETS[1], 0.01)], per_site_x="all")


def test_argument_rules():
    g = golden("chain_golden.npz")
    st = two_sites(g)
    jt = bh.JointTarget(slots_of(g, X_SETS[0]))
    # a sequence without SiteTargets
    with pytest.raises(ValueError, match="a sequence of modelpriors dicts needs SiteTargets"):
        DeviceChains(jt, 2, None, [dict(vs=(2, 5))])
    with pytest.raises(ValueError, match="a sequence of initparams dicts needs SiteTargets"):
        DeviceChains(jt, 2, [dict(lvz=0.1)], None)
    with pytest.raises(ValueError, match="prior_table=True needs SiteTargets"):
        DeviceChains(jt, 2, None, None, prior_table=True)
    # the length of a sequence
    with pytest.raises(ValueError, match="3 modelpriors dicts for 2 sites"):
        DeviceChains(st, 2, None, [{}, {}, {}])
    with pytest.raises(ValueError, match="1 initparams dicts for 2 sites"):
        DeviceChains(st, 2, [{}], None)
    # keys the sites share: the key and the site are named
    other = dict(iter_burnin=100, iter_main=7, maxmodels=3, rcond=1e-5, savepath="elsewhere/")
    assert sorted(other) == sorted(SHARED_INITPARAMS)
    for key, v in other.items():
        with pytest.raises(ValueError, match=r"initparams\['%s'\] of site 1 is .*, site 0's .*: the sites of one run share it" % key):
            DeviceChains(st, 2, [{}, {key: v}], None)
        site_dicts([{key: v}, {key: v}], None, 2, True)          # the same value everywhere is fine
    # a site's layers beyond the engine's capacity, with the site named
    with pytest.raises(E.EngineError, match=r"site 1: priors\['layers'\]\[1\] \+ 1 = 33 exceeds BH_CHAIN_MAXLAYERS = 32"):
        DeviceChains(st, 2, None, [dict(layers=(1, 20)), dict(layers=(1, 32))])
    site_dicts(None, [dict(layers=(1, 20)), dict(layers=(1, 31))], 2, True)
    with pytest.raises(E.EngineError, match=r"^priors\['layers'\]\[1\] \+ 1 = 33 exceeds"):
        DeviceChains(jt, 2, None, dict(layers=(1, 32)))


def test_equal_dicts_select_the_path_without_a_table():
    # one dict, none, or dicts whose MERGED contents agree in what the sampler reads: no table
    for ip, pr in ((None, None), (dict(lvz=0.1), dict(vs=(2, 5))), ([dict(lvz=0.1)] * 3, [dict(vs=(2, 5))] * 3),
                   ([{}, dict(thickmin=0.), dict(acceptance=(40, 45))], [dict(vs=(1, 5)), {}, dict(mantle=None)]),
                   ([dict(station="a"), dict(station="b"), dict(nchains=7)], None)):
        ips, prs, differ = site_dicts(ip, pr, 3, True)
        assert not differ and len(ips) == len(prs) == 3
        assert all(set(d) == set(DEFAULT_INITPARAMS) for d in ips) and all(set(d) == set(DEFAULT_PRIORS) for d in prs)
    # every modelpriors key and the site keys of initparams select it
    samples = dict(mantle=(4.2, 1.8), vpvs=1.73, layers=(1, 8), vs=(2, 4), z=(0, 40), mohoest=(30, 3), rfnoise_corr=0.5,
                   rfnoise_sigma=(1e-4, 0.01), swdnoise_corr=(0.1, 0.2), swdnoise_sigma=0.02)
    assert sorted(samples) == sorted(DEFAULT_PRIORS)
    for k, v in samples.items():
        assert site_dicts(None, [{}, {k: v}], 2, True)[2], k
    isamples = dict(propdist=(0.02, 0.02, 0.01, 0.005, 0.005), acceptance=(30, 50), thickmin=0.2, lvz=0.1, hvz=0.3)
    assert sorted(isamples) == sorted(SITE_INITPARAMS)
    for k, v in isamples.items():
        assert site_dicts([{}, {k: v}], None, 2, True)[2], k
    # merged over the defaults: a site's dict needs only what differs
    ips, prs, _ = site_dicts([{}, dict(lvz=0.1)], [dict(vs=(2, 4)), {}], 2, True)
    assert prs[0]["vs"] == (2, 4) and prs[1]["vs"] == DEFAULT_PRIORS["vs"] and prs[0]["z"] == DEFAULT_PRIORS["z"]
    assert ips[1]["lvz"] == 0.1 and ips[0]["lvz"] is None and ips[1]["propdist"] == DEFAULT_INITPARAMS["propdist"]


def test_a_sites_record_holds_that_sites_values():
    ips, prs, differ = site_dicts(
        [dict(thickmin=0.1, lvz=0.1, hvz=None, acceptance=(40, 80)), dict(thickmin=0.3, lvz=None, hvz=0.5, acceptance=(10, 20))],
        [dict(layers=(1, 20), vs=(2, 5), z=(0, 60), vpvs=(1.4, 2.1), mantle=None),
         dict(layers=(2, 8), vs=(2.5, 4.5), z=(1, 50), vpvs=1.73, mantle=(4.2, 1.8))], 2, True)
    assert differ
    noise = [[0.0, (1e-5, 0.1), (0.35, 0.75), (1e-5, 0.05)], [0.0, 0.03, (0.2, 0.6), np.float64(0.01)]]
    a, b = (set_station_fields(E.ChainPrior(), ips[s], prs[s], noise[s]) for s in range(2))
    assert (a.layermin, a.layermax, a.vsmin, a.vsmax, a.zmin, a.zmax) == (1, 20, 2.0, 5.0, 0.0, 60.0)
    assert (b.layermin, b.layermax, b.vsmin, b.vsmax, b.zmin, b.zmax) == (2, 8, 2.5, 4.5, 1.0, 50.0)
    assert (a.thickmin, a.lvz, a.hvz, a.acc_lo, a.acc_hi) == (0.1, 0.1, -1.0, 40.0, 80.0)       # None -> -1
    assert (b.thickmin, b.lvz, b.hvz, b.acc_lo, b.acc_hi) == (0.3, -1.0, 0.5, 10.0, 20.0)
    assert (a.vpvsmin, a.vpvsmax, a.mantle_vs, a.mantle_vpvs) == (1.4, 2.1, -1.0, 0.0)
    assert (b.vpvsmin, b.vpvsmax, b.mantle_vs, b.mantle_vpvs) == (1.73, 1.73, 4.2, 1.8)          # fixed: lo == hi
    assert list(a.noise_lo)[:4] == [0.0, 1e-5, 0.35, 1e-5] and list(a.noise_hi)[:4] == [0.0, 0.1, 0.75, 0.05]
    assert list(b.noise_lo)[:4] == [0.0, 0.03, 0.2, 0.01] and list(b.noise_hi)[:4] == [0.0, 0.03, 0.6, 0.01]
    assert not any(list(a.noise_lo)[4:]) and not any(list(b.noise_hi)[4:])                      # beyond 2 nt: fixed at 0
    # the same function fills a bh_chain_config's station fields (the path without a table)
    c = set_station_fields(E.ChainConfig(), ips[1], prs[1], noise[1])
    for k, _ in E.ChainPrior._fields_:
        u, v = getattr(b, k), getattr(c, k)
        assert (list(u) == list(v)) if k.startswith("noise_") else (u == v), k


def test_engine_methods_pass_the_table_to_the_new_entry_points():
    class Lib(object):
        def __init__(self):
            self.calls = []

        def bh_chain_propose_window_priors(self, *a):
            self.calls.append(("propose", a[7:]))
            return 0

        def bh_chain_accept_window_priors(self, *a):
            self.calls.append(("accept", a[7:]))
            return E.BH_EINVAL

        def bh_engine_stream(self, h):
            return None

    eng = E.Engine.__new__(E.Engine)
    eng._L, eng._h = Lib(), None
    cfg, st = E.ChainConfig(), E.ChainState()
    eng.chain_propose_window_priors(cfg, st, 4, 0, 1, 4, 111, 2, 222)
    eng.chain_propose_window_priors(cfg, st, 4, 0, 1, 4, 111, 2, 222, absent=333)
    assert eng._L.calls == [("propose", (111, 2, 222, None)), ("propose", (111, 2, 222, 333))]
    with pytest.raises(E.EngineError, match="bh_chain_accept_window_priors failed"):
        eng.chain_accept_window_priors(cfg, st, 4, 0, 1, 4, 5, 6, 111, 2, 222)
    assert eng._L.calls[-1] == ("accept", (5, 6, 111, 2, 222))
