"""The CPU oracle (oracle/swd_oracle.c) against the reference: golden vectors produced by the
reference's own SurfDisp.run_model + compiled surfdisp96.f (tests/golden/gen_golden.py) and the
reference's own tutorial files st3_*.dat.  These pin the oracle (-m "not gpu")."""
import numpy as np
import pytest

from conftest import golden, st3

REFS = {"rdispph": (2, 0), "rdispgr": (2, 1), "ldispph": (1, 0), "ldispgr": (1, 1)}


def run(oracle, h, vp, vs, rho, per, iwave, igr, mode=1, flsph=0):
    cg = np.zeros(per.size)
    err = oracle.surfdisp96(h, vp, vs, rho, h.size, flsph, iwave, mode, igr, per.size, per, cg)
    return err, cg


@pytest.mark.parametrize("pset", ["p21", "p30"])
def test_oracle_matches_reference_golden(oracle, pset):
    g = golden("swd_golden.npz")
    per = g["x_" + pset]
    nbad = 0
    for im in range(g["nlay"].size):
        n = g["nlay"][im]
        for ir, ref in enumerate(g["refs"]):
            iwave, igr = REFS[str(ref)]
            err, cg = run(oracle, g["h"][im, :n], g["vp"][im, :n], g["vs"][im, :n], g["rho"][im, :n], per, iwave, igr)
            assert (err == 0) == bool(g["ok_" + pset][im, ir])
            if err == 0:
                # gate of SURVEY.md 7.2 is 1e-9 / 1e-6; the restatement is in fact bit-identical
                assert np.array_equal(cg, g["y_" + pset][im, ir]), (im, ref)
            else:
                nbad += 1
    assert nbad > 0  # the fixture contains models surf96 fails on


def test_oracle_resampling_path_inputs(oracle):
    """>60 periods: the reference computes on linspace-60 and interpolates (surf96_modsw.py:35-43)."""
    g = golden("swd_golden.npz")
    per = g["x_p80"]
    p60 = np.linspace(per.min(), per.max(), 60)
    for im in (0, 5, 72):
        n = g["nlay"][im]
        for ir, ref in enumerate(g["refs"]):
            if not g["ok_p80"][im, ir]:
                continue
            iwave, igr = REFS[str(ref)]
            err, cg = run(oracle, g["h"][im, :n], g["vp"][im, :n], g["vs"][im, :n], g["rho"][im, :n], p60, iwave, igr)
            assert err == 0
            assert np.array_equal(np.interp(per, p60, cg), g["y_p80"][im, ir])


@pytest.mark.parametrize("tag,kw", [("mode2", dict(mode=2)), ("sph", dict(flsph=1))])
def test_oracle_options(oracle, tag, kw):
    g = golden("swd_golden.npz")
    per = g["x_p30"]
    for jj, im in enumerate(g["sub_idx"]):
        n = g["nlay"][im]
        for ir, ref in enumerate(g["refs"]):
            iwave, igr = REFS[str(ref)]
            err, cg = run(oracle, g["h"][im, :n], g["vp"][im, :n], g["vs"][im, :n], g["rho"][im, :n], per, iwave, igr, **kw)
            assert (err == 0) == bool(g["ok_" + tag][jj, ir])
            if err == 0:
                assert np.array_equal(cg, g["y_" + tag][jj, ir])


@pytest.mark.parametrize("ref", sorted(REFS))
def test_oracle_matches_tutorial_files(oracle, ref):
    """tutorial/observed/st3_*.dat: 4-decimal files written by the reference's own forward code."""
    x, y = st3(ref)
    h = np.array([5., 23., 8., 0.]); vs = np.array([2.7, 3.6, 3.8, 4.4]); vp = vs * 1.73
    err, cg = run(oracle, h, vp, vs, vp * 0.32 + 0.77, x, *REFS[ref])
    assert err == 0
    assert np.max(np.abs(cg - y)) <= 5.1e-5


COMPILED_PERIODS = np.linspace(2, 60, 30)


def compiled_reference_cases():
    """The random inputs of the bit-equality test against the compiled reference (its outputs on them are stored in
    tests/golden/compiled_golden.npz by `tests/golden/gen_golden.py compiled`): 60 models, then 200 arguments of the
    secular functions (om, c, h, vp, vs, rho)."""
    rs = np.random.RandomState(5)
    models, secular = [], []
    for it in range(60):
        L = rs.randint(2, 22)
        vs = np.sort(rs.uniform(2.0, 4.8, L))
        if it % 4 == 0 and L > 3:
            vs[rs.randint(1, L - 1)] *= 0.85
        h = rs.uniform(0.5, 8, L); h[-1] = 0
        vp = vs * rs.uniform(1.5, 2.0); rho = 0.32 * vp + 0.77
        models.append((h, vp, vs, rho))
    for _ in range(200):
        L = rs.randint(2, 12)
        vs = np.sort(rs.uniform(2.0, 4.8, L)); h = rs.uniform(0.5, 8, L); vp = vs * 1.75; rho = 0.32 * vp + 0.77
        om = 2 * np.pi / rs.uniform(1, 60); c = rs.uniform(1.7, 5.0)
        secular.append((om, c, h, vp, vs, rho))
    return models, secular


def test_oracle_matches_compiled_reference_random(oracle):
    """Bit-equality with the compiled reference on random models: against its stored outputs, and where oracle/_ref is
    built, against the reference itself as well."""
    from oracle import refshim
    g = golden("compiled_golden.npz")
    live = refshim.available()
    models, secular = compiled_reference_cases()
    per = COMPILED_PERIODS
    for i, (h, vp, vs, rho) in enumerate(models):
        for j, (iwave, igr) in enumerate(REFS.values()):
            a = np.zeros(30)
            ea = oracle.surfdisp96(h, vp, vs, rho, h.size, 0, iwave, 1, igr, 30, per, a)
            assert ea == g["swd_err"][i, j] and np.array_equal(a, g["swd_vel"][i, j]), (i, j)
            if live:
                b = np.zeros(30)
                eb = refshim.surfdisp96(h, vp, vs, rho, h.size, 0, iwave, 1, igr, 30, per, b)
                assert ea == eb and np.array_equal(a, b)
    for i, (om, c, h, vp, vs, rho) in enumerate(secular):
        for j, ifunc in enumerate((1, 2)):
            d = oracle.dltar(om / c, om, ifunc, h, vp, vs, rho)
            assert d == g["dltar"][i, j], (i, j)
            if live:
                assert d == refshim.dltar(om / c, om, ifunc, h, vp, vs, rho)


def test_short_refinement_restatement_stays_within_tolerance_of_the_reference(oracle):
    """`oracle.swd_search(True)` = the CPU restatement of the engine's short root refinement (its default search)
    (bh_engine_set_swd_search; swd_common.h) -- not the reference's algorithm.  Its gate, on the CPU: phase velocities
    within north_star's 1e-5 relative (achieved: 1.2e-6) of the reference's golden vectors and of the reference
    sequence on random models, the same models failing, fewer evaluations; group velocities untouched."""
    from bayhunter_amd.synth import synth_models
    g = golden("swd_golden.npz")
    nlay = g["nlay"]
    a = [np.ascontiguousarray(g[k], dtype=np.float64) for k in ("h", "vp", "vs", "rho")]
    for pset in ("p21", "p30"):
        per = g["x_" + pset]
        for ir, ref in enumerate(g["refs"]):
            iwave, igr = REFS[str(ref)]
            with oracle.swd_search(True):
                v, e, _ = oracle.swd_batch(nlay, *a, per, iwave, igr)
            ok = g["ok_" + pset][:, ir].astype(bool)
            y = g["y_" + pset][:, ir]
            assert np.array_equal(e == 0, ok)
            assert np.max(np.abs(v[ok] - y[ok]) / y[ok]) <= (1e-5 if igr == 0 else 0.0)
    rs = np.random.RandomState(2024)
    nlay, h, vp, vs, rho = synth_models(rs, 3000, 12, lvz_frac=0.25, ragged=True)
    per = np.linspace(2, 60, 30)
    a = [np.ascontiguousarray(x.T) for x in (h, vp, vs, rho)]
    for iwave in (2, 1):
        ov, oe, nref = oracle.swd_batch(nlay, *a, per, iwave, 0)
        with oracle.swd_search(True):
            v, e, nfast = oracle.swd_batch(nlay, *a, per, iwave, 0)
        assert np.array_equal(e, oe)
        both = (v != 0) & (ov != 0)
        assert np.max(np.abs(v[both] - ov[both]) / ov[both]) <= 1.2e-6
        assert np.array_equal(v[oe == 0] == 0, ov[oe == 0] == 0)
        assert nfast < 0.8 * nref
    v0, _, n0 = oracle.swd_batch(nlay, *a, per, 1, 0)                # (the switch is off again)
    assert np.array_equal(v0, ov) and n0 == nref


def test_love_mode_count_is_monotone_and_consistent_with_the_sign_of_the_secular_function(oracle):
    """bho_dltar1_count (the restatement of swd_common.h's LoveCount): N(c) = sign changes of dltar1 below c.  On a fine
    velocity grid N never decreases, it changes parity exactly where the function changes sign, and the value returned is
    dltar1's bit for bit -- LVZ-rich models, 1 to 60 s."""
    import ctypes as C
    from bayhunter_amd.synth import synth_models
    L = oracle.lib()
    fp = C.POINTER(C.c_float)
    L.bho_dltar1_count.restype = C.c_double
    L.bho_dltar1_count.argtypes = [C.c_double, C.c_double, fp, fp, fp, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    rs = np.random.RandomState(5)
    nlay, h, vp, vs, rho = synth_models(rs, 40, 12, lvz_frac=0.4, ragged=True)
    pairs = 0
    for b in range(40):
        n = int(nlay[b])
        d, bb, r = [np.ascontiguousarray(x[:n, b], dtype=np.float32) for x in (h, vs, rho)]
        for T in (1.0, 3.0, 11.0, 60.0):
            om = 2 * np.pi / T
            prev = None
            for c in np.linspace(0.5 * float(bb.min()), float(bb[-1]) * 0.99999, 1500):
                cnt, val = C.c_int(), C.c_int()
                f = L.bho_dltar1_count(om / c, om, d.ctypes.data_as(fp), bb.ctypes.data_as(fp), r.ctypes.data_as(fp), n, 1,
                                       C.byref(cnt), C.byref(val))
                assert f == L.bho_dltar1(om / c, om, d.ctypes.data_as(fp), bb.ctypes.data_as(fp), r.ctypes.data_as(fp), n, 1)
                if prev is not None and val.value and prev[2]:
                    assert cnt.value >= prev[0]
                    assert ((cnt.value - prev[0]) % 2 == 1) == (np.signbit(f) != np.signbit(prev[1]))
                    pairs += 1
                prev = (cnt.value, f, val.value)
    assert pairs > 200000


def test_counted_scan_finds_the_reference_brackets(oracle):
    """Scan mode 1 (the engine's default; swd_common.h: the counted scan) against getsol's step-by-step scan: the SAME
    velocities and failure flags, bit for bit, with fewer evaluations -- reference refinement and short refinement, Love
    phase / group, higher modes, earth flattening, thin and deep LVZ-rich models; Rayleigh unaffected."""
    from bayhunter_amd.synth import synth_models
    per = np.linspace(2, 60, 30)
    cases = [(2024, 4000, 12, 1, 0, 1, 0, per), (7, 6000, 4, 1, 0, 1, 0, np.array([0.5, 1, 2, 3, 5, 8, 13, 21, 34, 55.])),
             (3, 1500, 12, 1, 0, 3, 0, per), (4, 1500, 12, 1, 1, 2, 0, per), (5, 1500, 12, 1, 0, 1, 1, per),
             (6, 400, 40, 1, 0, 1, 0, np.linspace(0.3, 40, 60)), (8, 500, 12, 2, 0, 1, 0, per),
             # higher modes whose previous root lies below the floor the previous mode sets (getsol moves the start to clow
             # first: the counted scan must step there -- found by tools/gpu_fuzz.py in round 4)
             (9, 6000, 8, 1, 1, 3, 0, np.sort(np.random.RandomState(9).uniform(1.0, 80.0, 30))),
             (10, 3000, 10, 1, 1, 3, 1, np.sort(np.random.RandomState(10).uniform(1.0, 80.0, 21)))]
    for seed, B, L, iwave, igr, mode, flsph, pp in cases:
        rs = np.random.RandomState(seed)
        nlay, h, vp, vs, rho = synth_models(rs, B, L, lvz_frac=0.3, ragged=True, hmin=0.2 if L > 20 else 1.5, hmax=3 if L > 20 else 8.0)
        a = [np.ascontiguousarray(x.T) for x in (h, vp, vs, rho)]
        for search in (0, 1):
            with oracle.swd_search(search):
                v0, e0, n0 = oracle.swd_batch(nlay, *a, pp, iwave, igr, mode=mode, flsph=flsph)
                with oracle.swd_scan(1):
                    v1, e1, n1 = oracle.swd_batch(nlay, *a, pp, iwave, igr, mode=mode, flsph=flsph)
            assert np.array_equal(v0, v1) and np.array_equal(e0, e1), (seed, search)
            if iwave == 1:
                assert n1 < 0.85 * n0, (seed, search, n0, n1)
            else:
                assert n1 == n0


def test_guarded_short_refinement_returns_the_reference_failure_flags(oracle):
    """Search mode 2 = what BH_SEARCH_FAST runs: the short refinement with its guard (swd_common.h).  Where the reference's
    own outcome hinges on the last bits of a previous root (a root and its mirror image around a half-space velocity closer
    together than a scan step; a bracket that contains betmx) the guard fires and the model is run again with the
    reference's sequence: failure flags AND the period from which a failed row is zero are the reference's on every model,
    velocities within 1e-5 (achieved 1.2e-6).  Thin models with long periods are where the unguarded sequence differs
    (here: some tens of rows)."""
    from bayhunter_amd.synth import synth_models
    per = np.linspace(2, 60, 30)
    nraw = 0
    for seed, B, L, iwave, mode in ((11, 60000, 4, 1, 1), (12, 20000, 12, 1, 1), (13, 6000, 12, 2, 1), (14, 8000, 6, 1, 2)):
        rs = np.random.RandomState(seed)
        nlay, h, vp, vs, rho = synth_models(rs, B, L, lvz_frac=0.25, ragged=True)
        a = [np.ascontiguousarray(x.T) for x in (h, vp, vs, rho)]
        with oracle.swd_scan(1):
            ov, oe, nref = oracle.swd_batch(nlay, *a, per, iwave, 0, mode=mode)
            with oracle.swd_search(1):
                rv, re_, _ = oracle.swd_batch(nlay, *a, per, iwave, 0, mode=mode)
            oracle.swd_guarded_count()
            with oracle.swd_search(2):
                gv, ge, ng = oracle.swd_batch(nlay, *a, per, iwave, 0, mode=mode)
            nguard = oracle.swd_guarded_count()
        nraw += int(((rv == 0) != (ov == 0)).any(axis=1).sum())
        assert np.array_equal(ge, oe), seed
        assert np.array_equal(gv == 0, ov == 0), seed
        both = (gv != 0) & (ov != 0)
        assert np.max(np.abs(gv[both] - ov[both]) / ov[both]) <= 1.2e-6
        if mode > 1:      # targets with higher modes keep the reference sequence: its bits, no guard
            assert nguard == 0 and np.array_equal(gv, ov) and np.array_equal(rv, ov)
        assert 0 < nguard < 0.3 * B or iwave == 2 or mode > 1
        assert ng < nref or iwave == 1 or mode > 1
    assert nraw > 10   # the unguarded sequence does differ on these sets


def group_velocity_sets():
    """(nlay, h, vp, vs, rho [model-major], periods) of the test below: golden models, sorted velocities with a low-velocity
    zone, models drawn from a sampler's prior."""
    from bayhunter_amd.synth import synth_models, prior_models
    g = golden("swd_golden.npz")
    sets = [(g["nlay"], g["h"], g["vp"], g["vs"], g["rho"], g["x_p30"])]
    rs = np.random.RandomState(314)
    for gen in (lambda: synth_models(rs, 150, 12, lvz_frac=0.4, ragged=True), lambda: prior_models(rs, 150, 21)):
        nlay, h, vp, vs, rho = gen()
        sets.append((nlay, h.T, vp.T, vs.T, rho.T, np.sort(rs.uniform(1.0, 70.0, 24))))
    return sets


def test_group_velocity_roots_in_the_device_order_are_the_reference_bits(oracle):
    """The device runs a fundamental-mode group velocity as the chain of its first roots (t/(1+h)) and then the second roots (t/(1-h))
    as independent searches (engine_swd.hip launch_swd_jobs): the second root of a period starts from the first root of
    the same period and from nothing else (surfdisp96.f:282-287).  The oracle in that order (last period first) against the
    reference's order: the same bits and flags -- golden models (with the models surf96 fails on), sorted velocities with a
    low-velocity zone, models drawn from a sampler's prior, flat and flattened, with and without the counted Love scan; and
    against the compiled reference: its stored outputs, and the reference itself where it is built."""
    from oracle import refshim
    sets = group_velocity_sets()
    nfail = 0
    for nlay, h, vp, vs, rho, per in sets:
        for iwave in (1, 2):
            for flsph in (0, 1):
                for counted in (0, 1):
                    with oracle.swd_scan(counted):
                        ov, oe, _ = oracle.swd_batch(nlay, h, vp, vs, rho, per, iwave, 1, flsph=flsph)
                        with oracle.swd_group_split():
                            sv, se, _ = oracle.swd_batch(nlay, h, vp, vs, rho, per, iwave, 1, flsph=flsph)
                    assert np.array_equal(se, oe) and np.array_equal(sv, ov), (iwave, flsph, counted)
                nfail += int(oe.sum())
    assert nfail > 0   # (models whose chain of first roots ends early are among them)
    nlay, h, vp, vs, rho, per = sets[1]
    with oracle.swd_group_split():
        sv, se, _ = oracle.swd_batch(nlay, h, vp, vs, rho, per, 2, 1)
    rows = np.arange(0, nlay.size, 5)
    c = golden("compiled_golden.npz")
    assert np.array_equal(se[rows], c["group_err"]) and np.array_equal(sv[rows], c["group_vel"])
    if refshim.available():
        for b in rows:
            n = int(nlay[b]); r = np.zeros(per.size)
            er = refshim.surfdisp96(h[b, :n], vp[b, :n], vs[b, :n], rho[b, :n], n, 0, 2, 1, 1, per.size, per, r)
            assert er == se[b] and np.array_equal(r, sv[b])
