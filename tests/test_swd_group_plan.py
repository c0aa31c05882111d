"""The group kernel's launch plan (bh_plan_swd_group, csrc/swd_group_kernel.hip), which needs no GPU: over the call shapes and
requests the engine can make, every plan names one of the builds the translation units compile, and every compiled build is
named by some plan.  Its decisions on the grid, the SIMD-pairing geometry and restart in place hold together."""
import ctypes as C
import itertools
import os
import re

from conftest import REPO

SRC = os.path.join(REPO, "bayhunter_amd", "csrc", "swd_group_kernel.hip")


class Target(C.Structure):
    _fields_ = [("K", C.c_int), ("look", C.c_int), ("iwave", C.c_int), ("mode", C.c_int), ("group", C.c_bool), ("refseq", C.c_bool)]


class Ask(C.Structure):  # SwdGroupAsk (bh_device.h)
    _fields_ = [("B", C.c_int), ("Lmax", C.c_int), ("Lcut", C.c_int), ("ntargets", C.c_int), ("G0", C.c_int), ("t", Target * 8),
                ("fast", C.c_bool), ("farith", C.c_bool), ("restart", C.c_bool), ("adapt_ok", C.c_bool), ("rerun", C.c_bool),
                ("counters", C.c_bool), ("scan", C.c_int)]


class Dim3(C.Structure):
    _fields_ = [("x", C.c_uint), ("y", C.c_uint), ("z", C.c_uint)]


class Build(C.Structure):  # SwdGroupBuild
    _fields_ = [("fastm", C.c_int), ("simple", C.c_bool), ("prof", C.c_bool), ("adapt", C.c_bool), ("cntb", C.c_bool), ("fa", C.c_bool)]


class Info(C.Structure):  # SwdLaunchInfo
    _fields_ = [("workgroups", C.c_uint), ("waves", C.c_long), ("lds", C.c_size_t), ("wpb", C.c_int)]


class Plan(C.Structure):  # SwdGroupPlan
    _fields_ = [("fits", C.c_bool), ("rows", C.c_int * 2), ("lanes", C.c_int * 2), ("wg_n0", C.c_int), ("wg_n1", C.c_int),
                ("wave_lds", C.c_size_t), ("lds", C.c_size_t), ("grid", Dim3), ("block", Dim3), ("Gflags", C.c_int),
                ("restart", C.c_bool), ("build", Build), ("pair", C.c_bool), ("pair_mpw", C.c_int * 2), ("pair_waves", C.c_int * 2),
                ("info", Info)]


def compiled_builds():
    """(FASTM, SIMPLE, PROF, ADAPT, CNTB, FA) of every launch_build<...> the translation units list."""
    src = open(SRC).read()
    out = []
    for args in re.findall(r"launch_build<([^>]*)>\(a, g, s\)", src):
        v = [x.strip() for x in args.split(",")]
        out.append((int(v[0]),) + tuple(x == "true" for x in v[1:]) + ((False,) if len(v) == 5 else ()))
    return out


def library():
    from bayhunter_amd import engine as E
    lib = C.CDLL(E.LIB_PATH)
    plan = lib._Z17bh_plan_swd_groupRK11SwdGroupAskRK8BhTuning
    plan.restype, plan.argtypes = Plan, [C.POINTER(Ask), C.c_void_p]
    tuning = lib._Z9bh_tuningv
    tuning.restype = C.c_void_p
    tset, tget = lib._Z13bh_tuning_setPKci, lib._Z13bh_tuning_getPKcPi
    tset.argtypes, tget.argtypes = [C.c_char_p, C.c_int], [C.c_char_p, C.POINTER(C.c_int)]
    return plan, tuning(), tset, tget


R, L = 2, 1
SETS = {  # (iwave, group velocity, mode) per target
    "R": [(R, False, 1)], "L": [(L, False, 1)], "RL": [(R, False, 1), (L, False, 1)], "RLg": [(R, False, 1), (L, True, 1)],
    "RgLg": [(R, True, 1), (L, True, 1)], "Rm2L": [(R, False, 2), (L, False, 1)],
}


def asks():
    """The main launches (three searches) and their re-runs, over shapes, lanes and the engine's requests."""
    for (B, Lmax, Lcut), name, G0, look in itertools.product([(1, 10, 10), (64, 10, 10), (4096, 10, 10), (2048, 21, 8), (64, 40, 40)],
                                                             SETS, (2, 4, 9), (1, 2, 7)):
        for search in ("reference", "fast", "fast_rayleigh"):
            tg = SETS[name]
            fast = [not g and m <= 1 and (search == "fast" or (search == "fast_rayleigh" and w == R)) for w, g, m in tg]
            for farith, adapt_ok, counters, scan, rerun in itertools.product((0, 1), (0, 1), (0, 1), (0, 1, 2), (0, 1)):
                if rerun and (not any(fast) or not adapt_ok or Lcut < Lmax):
                    continue
                q = Ask(B=B, Lmax=Lmax, Lcut=Lcut, ntargets=len(tg), G0=G0, farith=bool(farith), adapt_ok=bool(adapt_ok),
                        counters=bool(counters), scan=scan, rerun=bool(rerun), fast=any(fast) and not rerun,
                        restart=not rerun)
                for t, (w, g, m) in enumerate(tg):
                    q.t[t] = Target(K=20, look=(64 // G0 if rerun else look), iwave=w, mode=m, group=g,
                                    refseq=any(fast) and not g and not fast[t])
                yield q


def test_every_plan_names_a_compiled_build_and_every_build_is_planned():
    builds = compiled_builds()
    assert len(builds) == len(set(builds)) == 33
    plan, tun, tset, tget = library()
    switches = [{}, {b"swd_no_adapt": 1}, {b"swd_no_simple": 1}, {b"swd_no_restart": 1}, {b"swd_no_mix": 1}]
    planned = set()
    n = 0
    for sw in switches:
        old = {}
        for k, v in sw.items():
            x = C.c_int(0)
            assert tget(k, C.byref(x)) == 0
            old[k] = x.value
            assert tset(k, v) == 0
        try:
            for q in asks():
                g = plan(C.byref(q), tun)
                assert g.fits
                b = g.build
                key = (b.fastm, b.simple, b.prof, b.adapt, b.cntb, b.fa)
                assert key in builds, key
                planned.add(key)
                n += 1
                two = q.Lcut < q.Lmax
                assert (g.grid.z == 2) == two and g.lanes[1] >= min(q.G0, 64)
                assert g.block.x == 128 and g.lds == g.info.lds and g.info.wpb == 2
                if g.wg_n1 > 0:  # two targets interleaved in a one-dimensional grid
                    assert q.ntargets == 2 and not two and not q.rerun and g.grid.y == 1 and g.info.waves == g.wg_n0 + g.wg_n1
                if g.pair:
                    assert g.grid.y == 1 and g.grid.z == 1 and not two
                    for t in range(q.ntargets):
                        assert g.pair_waves[t] * g.pair_mpw[t] >= q.B > (g.pair_waves[t] - 1) * g.pair_mpw[t]
                if g.restart:
                    assert b.adapt and b.fastm == 1 and q.fast and not q.rerun
                if b.fa:
                    assert b.fastm == 2 and q.farith
                if q.rerun:
                    assert b.fastm == 0 and not g.restart and g.wg_n1 == 0
        finally:
            for k, v in old.items():
                tset(k, v)
    assert n > 10000
    assert planned == set(builds), sorted(set(builds) - planned)


def test_a_class_too_deep_for_a_workgroup_does_not_fit():
    plan, tun, _, _ = library()
    q = Ask(B=64, Lmax=1000, Lcut=1000, ntargets=1, G0=2, restart=True, adapt_ok=True)
    q.t[0] = Target(K=60, look=1, iwave=R, mode=3)
    assert not plan(C.byref(q), tun).fits
    q.Lmax = q.Lcut = 10
    assert plan(C.byref(q), tun).fits
