"""The device record of the chains' thinned samples (include/bh_engine_chain_record.h, DeviceChains(record="device")), the parts
that need no GPU: the snapshot arithmetic against a plain enumeration of run()'s loop, the header, the library's exports and the
ctypes mirror of the store, and what the constructor refuses before it touches the GPU."""
import ctypes
import os
import re

import pytest

from conftest import REPO
from bayhunter_amd import engine as E
from bayhunter_amd.device_chains import DeviceChains, record_rows, snapshot_count

THINNINGS = (1, 2, 7, 1000)
BURNINS = (0, 1, 6, 7, 14, 15, 1000, 1150, 2001)       # multiples of each thinning, and not
MAINS = (1, 7, 13, 250, 1000, 1001)


def run_loop(iter_burnin, iter_main, thinning, stop=None):
    """the iterations at which run() takes a snapshot (its present loop, one iteration at a time) -> (those < 0, those >= 0)"""
    p1, p2 = [], []
    i = -iter_burnin
    while i < (iter_main if stop is None else min(stop, iter_main)):
        if i % thinning == 0:
            (p1 if i < 0 else p2).append(i)
        i += 1
    return p1, p2


@pytest.mark.parametrize("thinning", THINNINGS)
def test_record_rows_are_the_snapshots_of_the_run_loop(thinning):
    for burnin in BURNINS:
        for main in MAINS:
            p1, p2 = run_loop(burnin, main, thinning)
            assert record_rows(burnin, main, thinning) == (len(p1), len(p2)), (burnin, main, thinning)
            assert snapshot_count(-burnin, main, thinning) == len(p1) + len(p2)


@pytest.mark.parametrize("thinning", THINNINGS)
def test_snapshot_count_gives_every_window_its_first_row(thinning):
    """row0 of a window that starts at iiter = the snapshots the loop took before it, for negative and positive iiter; and the
    count inside any window of up to 7 iterations"""
    for burnin in (6, 7, 15, 1150, 2001):
        due = [i for i in range(-burnin, 40) if i % thinning == 0]
        for iiter in list(range(-burnin, min(-burnin + 30, 0))) + list(range(-16, 40)) + [-1000, -999, -1001, 999, 1000, 1001]:
            if iiter < -burnin:
                continue
            before = sum(1 for i in range(-burnin, iiter) if i % thinning == 0)
            assert snapshot_count(-burnin, iiter, thinning) == before, (burnin, iiter, thinning)
            if iiter < 33:
                for depth in range(1, 8):
                    inside = [i for i in due if iiter <= i < iiter + depth]
                    assert snapshot_count(iiter, iiter + depth, thinning) == len(inside), (iiter, depth, thinning)
    assert snapshot_count(5, 5, thinning) == 0 and snapshot_count(5, 2, thinning) == 0
    assert snapshot_count(-2 * thinning, 2 * thinning + 1, thinning) == 5
    with pytest.raises(ValueError):
        snapshot_count(0, 10, 0)


def test_record_must_be_host_or_device():
    """refused first of all: no targets are looked at, nothing touches the GPU (this test runs without one)"""
    for bad in ("gpu", "Device", None, True, 1, ""):
        with pytest.raises(ValueError, match="record must be"):
            DeviceChains(None, 4, record=bad)


def header_text(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", name)).read(), flags=re.S)


def test_library_exports_the_record_header():
    raw = open(os.path.join(REPO, "include", "bh_engine_chain_record.h")).read()
    assert '#include "bh_engine_sites_priors.h"' in raw
    txt = header_text("bh_engine_chain_record.h")
    decl = sorted(set(re.findall(r"\b(bh_[a-z_]+)\s*\(", txt)))
    assert decl == ["bh_chain_accept_window_priors_record", "bh_chain_accept_window_record"]
    assert sorted(E.CHAIN_RECORD_SYMBOLS) == decl
    for other in (E.EXPORTED_SYMBOLS, E.DEBUG_SYMBOLS, E.SITE_SYMBOLS, E.SITE_RF_SYMBOLS, E.SITE_X_SYMBOLS, E.SITE_X_ALL_SYMBOLS,
                  E.SITE_MISSING_SYMBOLS, E.SITE_GAUSS_SYMBOLS, E.SITE_RF_AXIS_SYMBOLS, E.SITE_LAWS_SYMBOLS, E.SITE_PRIORS_SYMBOLS,
                  E.POSTERIOR_SYMBOLS):
        assert not set(decl) & set(other)
    lib = ctypes.CDLL(E.LIB_PATH)
    for name in decl:
        assert hasattr(lib, name), "missing export %s" % name
    for hdr in sorted(os.listdir(os.path.join(REPO, "include"))):           # declared in the new header only
        if hdr != "bh_engine_chain_record.h":
            assert "bh_chain_record" not in header_text(hdr) and "_record" not in header_text(hdr), hdr
    lib.bh_abi_version.restype = ctypes.c_int
    assert lib.bh_abi_version() == 10                            # extension headers are outside the contract


def test_the_ctypes_store_mirrors_the_header():
    txt = header_text("bh_engine_chain_record.h")
    body = re.search(r"typedef struct bh_chain_record \{(.*?)\} bh_chain_record;", txt, flags=re.S).group(1)
    fields = [(nm.strip().lstrip("*"), ctype + ("*" if "*" in nm else "")) for ctype, nm in re.findall(r"\b(float|double|int64_t)\s+([^;]+);", body)]
    mirror = [(k, "int64_t" if t is ctypes.c_int64 else "*") for k, t in E.ChainRecord._fields_]
    assert [f[0] for f in fields] == [m[0] for m in mirror]
    for (k, ctype), (_, kind) in zip(fields, mirror):
        assert ctype.endswith("*") == (kind == "*"), k
    assert ctypes.sizeof(E.ChainRecord) == 9 * 8
    assert [k for k, _ in E.ChainRecord._fields_][:6] == ["models", "likes", "vpvs", "misfits", "noise", "beta"]
