"""The receiver function's launch plan (bh_plan_rf, csrc/rf_plan.hip), which needs no GPU: over the shapes, builds, placements and
switches the engine can ask with, every field of the plan equals a restatement written here from csrc/rf_plan.h and DESIGN.md
(no code shared with the library), the plan's logm and jcut are those of a site's axis record (bh_rf_axis_record), every kernel a
plan names is launched by the translation unit of its build, and every kernel a unit launches is named by some plan."""
import ctypes as C
import itertools
import math
import os
import re

from conftest import REPO

SRC = os.path.join(REPO, "bayhunter_amd", "csrc", "rf_kernel.hip")

OK, EUNSUPPORTED = 0, -4                                     # include/bh_engine.h
PLAIN, SITES, MISSING, SITEAXIS = range(4)                   # RfBuild
L16S, L32S, L16, L32, SERIAL = range(5)                      # RfCoefKernel
W4, W3, LONG = range(3)                                      # RfSynthKernel
REFUSE_NONE, REFUSE_NSAMP, REFUSE_SITE_LDS, REFUSE_ALLOWANCE = range(4)
KIB = 1024
NSAMP_TEXT = b"receiver function: nsamp above 262144 is not supported"


class Ask(C.Structure):  # RfAsk (rf_plan.h)
    _fields_ = [("B", C.c_int), ("Lmax", C.c_int), ("build", C.c_int), ("nsamp", C.c_int), ("fsamp", C.c_double), ("gauss", C.c_double),
                ("beside_swd", C.c_bool), ("gated", C.c_bool), ("rf_lds_beside_swd", C.c_int)]


class Plan(C.Structure):  # RfPlan
    _fields_ = [("code", C.c_int), ("refusal", C.c_int), ("coef", C.c_int), ("coef_grid", C.c_uint), ("synth", C.c_int), ("block", C.c_uint),
                ("lds", C.c_size_t), ("big_lds", C.c_bool), ("workspace", C.c_bool), ("work_bytes", C.c_size_t), ("logm", C.c_int),
                ("jcut", C.c_int), ("no_realc", C.c_int), ("no_rot", C.c_int), ("no_cut", C.c_int)]

    def key(self):
        return tuple(getattr(self, f) for f, _ in self._fields_)


class AxisRec(C.Structure):  # RfAxisRec
    _fields_ = [("fsamp", C.c_double), ("tshift", C.c_double), ("gauss", C.c_double), ("nsamp", C.c_int32), ("logm", C.c_int32),
                ("jcut", C.c_int32), ("pad", C.c_int32)]


def library():
    from bayhunter_amd import engine as E
    lib = C.CDLL(E.LIB_PATH)
    plan = lib._Z10bh_plan_rfRK5RfAskRK8BhTuning
    plan.restype, plan.argtypes = Plan, [C.POINTER(Ask), C.c_void_p]
    record = lib._Z17bh_rf_axis_recordiddd
    record.restype, record.argtypes = AxisRec, [C.c_int, C.c_double, C.c_double, C.c_double]
    text = lib._Z18bh_rf_refusal_texti
    text.restype, text.argtypes = C.c_char_p, [C.c_int]
    tuning = lib._Z9bh_tuningv
    tuning.restype = C.c_void_p
    tset, tget = lib._Z13bh_tuning_setPKci, lib._Z13bh_tuning_getPKcPi
    tset.argtypes, tget.argtypes = [C.c_char_p, C.c_int], [C.c_char_p, C.POINTER(C.c_int)]
    return plan, record, text, tuning(), tset, tget


class switched:
    """The switches of bh_tuning.h set for a block, and put back."""

    def __init__(self, tset, tget, sw):
        self.tset, self.tget, self.sw, self.old = tset, tget, sw, {}

    def __enter__(self):
        for k, v in self.sw.items():
            x = C.c_int(0)
            assert self.tget(k.encode(), C.byref(x)) == 0
            self.old[k] = x.value
            assert self.tset(k.encode(), v) == 0

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.tset(k.encode(), v)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def lds_of_trace(nsamp):
    """Half-length complex spectrum, the Nyquist bin, 64 twiddles and nsamp / 128 (at least one) more, 16 bytes each."""
    return 16 * (nsamp // 2 + 1 + 64 + max(nsamp // 128, 1))


def axis_cut(nsamp, fsamp, gauss):
    """logm: the half-length transform's 2^logm points; jcut: the first bin whose Gauss factor exp(-(w/a)^2 / 4) is below 1e-17
    (w / a beyond 12.5132), nsamp / 2 + 1 where no bin up to the Nyquist one is."""
    half = nsamp // 2
    logm = max(half - 1, 0).bit_length()
    dw = 2.0 * math.pi * fsamp / nsamp
    jc = math.floor(12.5132 * gauss / dw) + 1.0
    return logm, (int(jc) if jc < half else half + 1)


def expected(q, sw):
    """The plan of an ask as a tuple in Plan's field order, under the switches sw."""
    need = lds_of_trace(q.nsamp)
    through_hbm = need > 160 * KIB
    if through_hbm and q.build == SITEAXIS:
        return (EUNSUPPORTED, REFUSE_SITE_LDS) + (0,) * 13
    if through_hbm and q.nsamp > 262144:
        return (EUNSUPPORTED, REFUSE_NSAMP) + (0,) * 13
    behind_gate = q.beside_swd and q.gated and not sw.get("rf_keep_floor", 0)
    if through_hbm:
        lds = need - 16 * (q.nsamp // 2)  # (no floor on the workspace form)
    elif not q.beside_swd:
        lds = need
    else:
        lds = max(need, sw.get("rf_lds_gated", 0) if behind_gate else q.rf_lds_beside_swd)
    small = behind_gate and not sw.get("rf_coef_big", 0)
    if q.Lmax > 32:
        coef, per_wg = SERIAL, 256
    elif q.Lmax > 16:
        coef, per_wg = (L32S if small else L32), 8
    else:
        coef, per_wg = (L16S if small else L16), 16
    synth = LONG if through_hbm else (W3 if sw.get("rf_waves", 0) == 3 else W4)
    block = 128 if (sw.get("rf_threads", 0) == 128 and synth != LONG) else 256
    no_cut = 1 if sw.get("rf_no_cut", 0) else 0
    no_realc, no_rot = (1 if sw.get("rf_no_realc", 0) else 0), (1 if sw.get("rf_no_rot", 0) else 0)
    logm, jcut = (0, 0) if q.build == SITEAXIS else axis_cut(q.nsamp, q.fsamp, q.gauss)
    if no_cut and q.build != SITEAXIS:
        jcut = q.nsamp // 2 + 1
    return (OK, REFUSE_NONE, coef, -(-q.B // per_wg), synth, block, lds, lds > 64 * KIB, through_hbm,
            q.B * (q.nsamp // 2) * 16 if through_hbm else 0, logm, jcut, no_realc, no_rot, no_cut)


# ---- the grid -------------------------------------------------------------------------------------------------------------------
BS = (1, 7, 8, 9, 15, 16, 17, 255, 256, 257, 4096)
LMAXS = (1, 16, 17, 32, 33, 100)
NSAMPS = (4, 64, 128, 2048, 4096, 8192, 16384, 32768, 262144, 524288)
PLACES = ((False, False), (True, False), (True, True))  # (beside_swd, gated): alone, beside and ungated, beside and gated
SWITCHES = [{}, {"rf_threads": 128}, {"rf_waves": 3}, {"rf_no_cut": 1}, {"rf_coef_big": 1}, {"rf_keep_floor": 1}, {"rf_lds_gated": 20000},
            {"rf_threads": 128, "rf_waves": 3}, {"rf_keep_floor": 1, "rf_lds_gated": 20000}, {"rf_coef_big": 1, "rf_lds_gated": 20000},
            {"rf_coef_big": 1, "rf_keep_floor": 1}, {"rf_no_cut": 1, "rf_threads": 128}, {"rf_waves": 3, "rf_lds_gated": 20000},
            {"rf_no_realc": 1}, {"rf_no_rot": 1}, {"rf_no_realc": 1, "rf_no_rot": 1, "rf_no_cut": 1}]
FLOORS = (40960, 0)  # the engine's rf_lds_beside_swd: its default, and none


def asks(floors=FLOORS):
    for B, Lmax, nsamp, build, (beside, gated), floor in itertools.product(BS, LMAXS, NSAMPS, range(4), PLACES, floors):
        yield Ask(B=B, Lmax=Lmax, build=build, nsamp=nsamp, fsamp=20.0, gauss=2.5, beside_swd=beside, gated=gated, rf_lds_beside_swd=floor)


def launched_kernels():
    """Per build the kernels its translation unit launches: {(build, 'coef' | 'synth', number): kernel name}, read from the kernel
    tables of rf_kernel.hip -- the launcher launches table entries only, which is asserted too."""
    src = open(SRC).read()
    tail = src[src.index("the launcher: the plan"):]
    # the launcher launches by the plan's numbers, never a kernel by name
    launches = re.findall(r"hipLaunchKernelGGL\(\(?([A-Za-z_0-9<>\[\]\.]+)", tail)
    assert sorted(launches) == ["COEF[p.coef]", "COEF_SITES[p.coef]", "SYNTH[p.synth]"], launches

    def tables(name):
        out = []
        for body in re.findall(r"\(\*const %s\[RF_[A-Z]+_KERNELS\]\)\([^)]*\) = \{([^}]*)\};" % name, tail):
            out.append([x.strip() for x in body.replace("\n", " ").split(",")] if body.strip() else [])
        return out
    synth, coef_sites, coef = tables("SYNTH"), tables("COEF_SITES"), tables("COEF")
    # the unit of the site axes states its synthesis kernels first, the other two share a statement; one table of site-indexed
    # coefficient kernels for all; the units of BH_RF_MISSING have no others
    assert len(synth) == 2 and len(coef_sites) == 1 and len(coef) == 2 and coef[0] == []
    assert tail.index("#if BH_RF_SITEAXIS") < tail.index("SYNTH[") and tail.index("#if BH_RF_MISSING\nvoid (*const COEF[") > 0
    renamed = dict(re.findall(r"#define (rf_synth_kernel\w*) (rf_synth_m_kernel\w*)", src))  # (the names of the BH_RF_MISSING unit)
    assert len(renamed) == 3
    defined = set(re.findall(r"__global__[^\n]*\bvoid (\w+)\(", src))
    out = {}
    for build, syn, plain in ((PLAIN, synth[1], coef[1]), (SITES, synth[1], None), (MISSING, [renamed[k] for k in synth[1]], None),
                              (SITEAXIS, synth[0], None)):
        for i, k in enumerate(syn):
            if k != "nullptr":
                assert (k in defined) or (k in renamed.values()), k
                out[(build, "synth", i)] = k
        for i, k in enumerate(plain if plain is not None else coef_sites[0]):
            assert re.sub(r"<\d+>", "", k) in defined, k
            out[(build, "coef", i)] = k
    return out


def test_every_field_of_every_plan_equals_the_restatement():
    plan, _, text, tun, tset, tget = library()
    units = launched_kernels()
    named = set()
    n = 0
    for sw in SWITCHES:
        with switched(tset, tget, sw):
            for q in asks():
                p = plan(C.byref(q), tun)
                assert p.key() == expected(q, sw), (sw, [getattr(q, f) for f, _ in q._fields_], p.key(), expected(q, sw))
                n += 1
                if p.code != OK:
                    assert q.nsamp == 524288 or (q.build == SITEAXIS and q.nsamp >= 32768)
                    continue
                assert p.lds <= 160 * KIB
                assert p.big_lds == (p.lds > 64 * KIB)
                assert p.workspace == (q.build != SITEAXIS and lds_of_trace(q.nsamp) > 160 * KIB) == (p.synth == LONG)
                if p.workspace:  # no floor on the workspace form: what the twiddles and the Nyquist bin need, whatever the placement
                    assert p.lds == lds_of_trace(q.nsamp) - 16 * (q.nsamp // 2) and p.block == 256 and not p.big_lds
                    assert p.work_bytes == q.B * (q.nsamp // 2) * 16
                assert q.build != SITEAXIS or p.synth != LONG
                assert p.coef_grid * {L16S: 16, L16: 16, L32S: 8, L32: 8, SERIAL: 256}[p.coef] >= q.B
                # the kernels the plan names are launched by its build's unit
                assert (q.build, "coef", p.coef) in units and (q.build, "synth", p.synth) in units, (q.build, p.coef, p.synth)
                named.update([(q.build, "coef", p.coef), (q.build, "synth", p.synth)])
    assert n > 100000
    # ... and every kernel a unit launches is named by some plan: 13 of rf_kernel.hip (10 + 3; RF_SITES shares the synthesis kernels
    # of RF_PLAIN), 8 with BH_RF_MISSING, 7 with BH_RF_SITEAXIS
    assert named == set(units), sorted(set(units) - named)
    assert len({units[k] for k in units if k[0] in (PLAIN, SITES)}) == 13
    assert sum(k[0] == MISSING for k in units) == 8 and sum(k[0] == SITEAXIS for k in units) == 7
    assert text(REFUSE_NONE) == b"" and text(REFUSE_NSAMP) == NSAMP_TEXT
    assert b"allowance" in text(REFUSE_ALLOWANCE) and text(REFUSE_SITE_LDS) not in (b"", NSAMP_TEXT)


def test_the_long_trace_and_the_site_axis_limits():
    plan, _, text, tun, _, _ = library()

    def one(build, nsamp, beside=False, gated=False):
        q = Ask(B=64, Lmax=10, build=build, nsamp=nsamp, fsamp=20.0, gauss=2.5, beside_swd=beside, gated=gated, rf_lds_beside_swd=40960)
        return plan(C.byref(q), tun)
    for build in (PLAIN, SITES, MISSING, SITEAXIS):  # the longest trace a workgroup's LDS holds: 134 160 B, with the allowance
        p = one(build, 16384)
        assert (p.code, p.lds, p.big_lds, p.workspace, p.synth) == (OK, 134160, True, False, W4)
        assert one(build, 2048).lds == 17680 and one(build, 2048, True, False).lds == 40960 and one(build, 2048, True, True).lds == 17680
    for build in (PLAIN, SITES, MISSING):  # beyond it, the shared axis goes through the workspace, up to 2^18 samples
        p = one(build, 32768)
        assert (p.code, p.workspace, p.synth, p.block, p.lds) == (OK, True, LONG, 256, 16 + 1024 + 256 * 16)
        assert one(build, 32768, True, False).lds == p.lds
        p = one(build, 262144)
        assert (p.code, p.workspace, p.lds, p.work_bytes) == (OK, True, 16 + 1024 + 2048 * 16, 64 * 131072 * 16)
        p = one(build, 524288)
        assert (p.code, p.refusal) == (EUNSUPPORTED, REFUSE_NSAMP) and text(p.refusal) == NSAMP_TEXT
    p = one(SITEAXIS, 32768)  # the sites' own axes have no workspace form
    assert (p.code, p.refusal) == (EUNSUPPORTED, REFUSE_SITE_LDS)


def test_the_plan_and_the_axis_record_cut_alike():
    plan, record, _, tun, tset, tget = library()
    # the axes of test_gpu_rf_paths.py::test_cutoff_regimes and c3's: the cut at bin 1, none (the first bin below 1e-17 lies beyond
    # the half: 159, 1019 and 1019 bins), and an ordinary cut
    axes = [(64, 20.0, 0.1), (64, 2.0, 2.5), (256, 5.0, 10.0), (512, 5.0, 5.0), (2048, 20.0, 2.5)]
    want = [(5, 1), (5, 33), (7, 129), (8, 257), (10, 510)]
    for (nsamp, fsamp, gauss), (logm, jcut) in zip(axes, want):
        r = record(nsamp, fsamp, -3.5, gauss)
        assert (r.fsamp, r.tshift, r.gauss, r.nsamp, r.pad) == (fsamp, -3.5, gauss, nsamp, 0)
        assert (r.logm, r.jcut) == axis_cut(nsamp, fsamp, gauss) == (logm, jcut)
        for build in (PLAIN, SITES, MISSING, SITEAXIS):
            q = Ask(B=12, Lmax=8, build=build, nsamp=nsamp, fsamp=fsamp, gauss=gauss, rf_lds_beside_swd=40960)
            p = plan(C.byref(q), tun)
            assert (p.logm, p.jcut) == ((0, 0) if build == SITEAXIS else (r.logm, r.jcut))
            with switched(tset, tget, {"rf_no_cut": 1}):
                p = plan(C.byref(q), tun)
                assert (p.logm, p.jcut, p.no_cut) == ((0, 0, 1) if build == SITEAXIS else (r.logm, nsamp // 2 + 1, 1))
    # the last bin a cut can name: jc = half - 1 is a cut, jc = half is none (w / a: 30.59 and 31.23 bins of 2 pi 20 / 64)
    for nsamp, fsamp, gauss in [(64, 20.0, 4.8), (64, 20.0, 4.9), (128, 5.0, 1.2), (4, 1.0, 0.1)]:
        r = record(nsamp, fsamp, 0.0, gauss)
        assert (r.logm, r.jcut) == axis_cut(nsamp, fsamp, gauss)
    assert record(64, 20.0, 0.0, 4.8).jcut == 31 and record(64, 20.0, 0.0, 4.9).jcut == 33
