"""Every launch path of the likelihood (csrc/like_kernel.hip, csrc/gauss_kernel.hip) against the extended-precision reference
of tests/like_ref.py, within its a priori bound times like_ref.FACTOR: the Gauss-law contraction in its 64 x 64 and 128 x 128
forms (K split over 1, 2 and 4 workgroups, empty column slabs) and the in-kernel mat-vec (no_mfma), the exponential law's
closed form up to |r| = 0.9999, the nocorr and scaled-error laws, like_small_kernel / like_kernel selection, eight targets,
per-target failure flags, and the likelihood of the engine's own synthetics (fused receiver-function sums included).

Residual rows differ in magnitude by up to 1e6 from model to model, so a row mixed up with another is far outside any bound."""
import numpy as np
import pytest

import like_ref as LR
from bayhunter_amd import engine as E

pytestmark = pytest.mark.gpu

B_EDGE = (1, 63, 64, 65, 127, 128, 129)
N_EDGE = (1, 16, 17, 63, 64, 65, 127, 128, 129, 1000, 1025)
N_LONG = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1024, 16385, 65536)
R_SET = (-0.9999, -0.5, 0.0, 0.35, 0.75, 0.99, 0.9999)
_MATS = {}


def gauss_matrix(kind, n):
    """(R^-1, logdet_r): "pinv" = the reference's pinv(0.92^((i-j)^2), rcond=1e-6) (Targets.py:150-160), entries up to ~1e6;
    "random" = a general dense, non-symmetric matrix (a Toeplitz R^-1 hides an index shift that moves both indices)."""
    key = (kind, n)
    if key not in _MATS:
        if kind == "pinv":
            idx = np.arange(n)
            R = 0.92 ** ((idx[:, None] - idx[None, :]).astype(float) ** 2)
            _MATS[key] = (np.linalg.pinv(R, rcond=1e-6), float(np.linalg.slogdet(R)[1]))
        else:
            rs = np.random.RandomState(1000 + n)
            _MATS[key] = (rs.normal(0, 1, (n, n)) * 10.0 ** rs.uniform(-1, 1, (n, 1)), 3.25)
    return _MATS[key]


def residuals(rs, B, n, smooth=False):
    """[B, n] residual rows whose magnitudes differ by up to 1e6 from model to model; smooth = random walks."""
    z = rs.normal(0, 1, (B, n))
    if smooth:
        z = np.cumsum(z, axis=1) / np.sqrt(n)
    return z * (10.0 ** rs.uniform(-3, 3, B))[:, None]


def user(law, n, yobs, **kw):
    d = {"kind": E.TARGET_USER, "law": law, "n": n, "yobs": yobs}
    d.update(kw)
    return d


def check(got, descs, ymod, noise, what, ld_rows=None):
    """got = (logL, misfits, err) of the engine: no failure, logL and all nt + 1 misfits within FACTOR x the bound."""
    logL, misf, err = got
    ref, rmisf, bound, mbound = LR.joint_ref(descs, ymod, noise, ld_rows=ld_rows)
    assert np.all(err == 0), what
    LR.assert_within(logL, ref, bound, what + ": logL")
    LR.assert_within(misf, rmisf, mbound, what + ": misfits")
    return bound


class tuned(object):
    """set_tuning(name, value) for a block; the previous value back in any case."""

    def __init__(self, eng, name, value):
        self.eng, self.name, self.value = eng, name, value

    def __enter__(self):
        self.before = self.eng.tuning(self.name)
        self.eng.set_tuning(self.name, self.value)

    def __exit__(self, *exc):
        self.eng.set_tuning(self.name, self.before)


def gauss_batch(rs, kind, B, n):
    rinv, ld = gauss_matrix(kind, n)
    yobs = rs.normal(0, 1, n)
    ymod = yobs + residuals(rs, B, n, smooth=bool(rs.randint(2)))
    noise = np.column_stack((np.full(B, 0.92), rs.uniform(0.01, 0.1, B)))
    return [user(E.LAW_GAUSS, n, yobs, rinv=rinv, logdet_r=ld)], ymod, noise


@pytest.mark.parametrize("kind", ["pinv", "random"])
@pytest.mark.parametrize("n", N_EDGE)
def test_gauss_contraction_both_tile_forms_at_edge_shapes(engine, kind, n):
    """B in {1, 63, 64, 65, 127, 128, 129} at this n, through the 64 x 64 form and the 128 x 128 form (forced; automatic
    selection gives the 64 form at all of these shapes).  (65, 1025) at 64 has nsplit = 17.  Both forms agree with each other
    within the bound, and a repeated call returns the same bits."""
    rs = np.random.RandomState(n)
    for B in B_EDGE:
        descs, ymod, noise = gauss_batch(rs, kind, B, n)
        engine.set_targets(descs)
        out = {}
        for tile in (128, 64):
            with tuned(engine, "gauss_tile", tile):
                out[tile] = engine.loglike_batch(ymod, noise)
                again = engine.loglike_batch(ymod, noise)
            what = "%s B=%d n=%d tile=%d" % (kind, B, n, tile)
            bound = check(out[tile], descs, ymod, noise, what)
            assert np.array_equal(again[0], out[tile][0]) and np.array_equal(again[1], out[tile][1]), what + ": not repeatable"
        LR.assert_within(out[64][0], out[128][0].astype(LR.LD), bound, "%s B=%d n=%d: 64 vs 128 form" % (kind, B, n))


@pytest.mark.parametrize("kind", ["pinv", "random"])
@pytest.mark.parametrize("tile,B,n", [(0, 8192, 200), (0, 4096, 1024), (0, 2048, 1024),   # automatic: 128 form, K split 1, 2, 4
                                      (64, 8192, 320), (128, 1, 520), (128, 129, 129)])
def test_gauss_contraction_launch_forms_at_large_shapes(engine, kind, tile, B, n):
    """Automatic selection where the 128 x 128 form runs with K over 1, 2 and 4 workgroups (big_ksplit); the 64 form forced at
    (8192, 320): nsplit = 4 slabs of 128 columns, the last one [384, 320) empty -- run right after the 128 form of the same
    shape, whose 12 slabs per model leave other values in the partial-sum buffer, so an empty slab must be written as 0; the
    128 form forced at (1, 520) (K split 4) and (129, 129).  Extended precision on sample_rows(), float64 BLAS elsewhere."""
    rs = np.random.RandomState(B + n)
    descs, ymod, noise = gauss_batch(rs, kind, B, n)
    engine.set_targets(descs)
    forms = [128, 64] if tile == 64 else [tile]
    for t in forms:
        with tuned(engine, "gauss_tile", t):
            got = engine.loglike_batch(ymod, noise)
            again = engine.loglike_batch(ymod, noise)
        what = "%s B=%d n=%d tile=%d" % (kind, B, n, t)
        check(got, descs, ymod, noise, what)
        assert np.array_equal(again[0], got[0]), what + ": not repeatable"


def test_gauss_in_kernel_matvec_no_mfma(engine):
    """no_mfma: like_kernel's LDS mat-vec instead of the contraction (the switch is read when an engine is created).  Against
    the reference and against the MFMA forms of the process-wide engine, at a subset of the edge shapes."""
    before = engine.tuning("no_mfma")
    engine.set_tuning("no_mfma", 1)
    eng = None
    try:
        eng = E.Engine(0)
        rs = np.random.RandomState(11)
        for kind in ("pinv", "random"):
            for n in (1, 17, 64, 65, 129, 1025):
                for B in (1, 64, 129):
                    descs, ymod, noise = gauss_batch(rs, kind, B, n)
                    what = "no_mfma %s B=%d n=%d" % (kind, B, n)
                    eng.set_targets(descs)
                    got = eng.loglike_batch(ymod, noise)
                    bound = check(got, descs, ymod, noise, what)
                    assert np.array_equal(eng.loglike_batch(ymod, noise)[0], got[0]), what + ": not repeatable"
                    engine.set_targets(descs)
                    for tile in (64, 128):
                        with tuned(engine, "gauss_tile", tile):
                            mf = engine.loglike_batch(ymod, noise)[0]
                        LR.assert_within(got[0], mf.astype(LR.LD), bound, what + ": vs the %d form" % tile)
    finally:
        if eng is not None:
            eng.close()
        engine.set_tuning("no_mfma", before)


@pytest.mark.parametrize("n", N_LONG)
def test_exponential_law_closed_form(engine, n):
    """((1+r^2) sum d^2 - r^2 edge - 2r sum d_i d_i+1) / (sigma^2 (1-r^2)) against the tridiagonal get_corr_inv, for every r of
    R_SET on white and on smooth (random-walk) residuals -- where a lost or doubled cross term shows most; n = 64 / 65 is the
    hand-over from like_small_kernel to like_kernel."""
    rs = np.random.RandomState(n + 1)
    yobs = rs.normal(0, 1, n)
    r = np.array(R_SET * 2)
    B = r.size
    ymod = yobs + np.vstack((residuals(rs, B // 2, n), residuals(rs, B - B // 2, n, smooth=True)))
    noise = np.column_stack((r, rs.uniform(0.01, 0.1, B)))
    descs = [user(E.LAW_EXP, n, yobs)]
    engine.set_targets(descs)
    check(engine.loglike_batch(ymod, noise), descs, ymod, noise, "exp n=%d" % n)


def scaled_yerr(rs, n, at):
    """yerr spanning 1e-3 .. 10 with its minimum at index `at`: most entries within 1e-3 (1 + 1e-3) of the minimum, up to 40
    spread log-uniformly to 10, so that prod(yerr / min) stays finite at n = 65536."""
    ye = 1e-3 * (1.0 + 1e-3 * rs.uniform(0.1, 1, n))
    k = min(max(n - 1, 0), 40)
    pos = rs.choice([i for i in range(n) if i != at], size=k, replace=False) if k else np.zeros(0, dtype=int)
    ye[pos] = 10.0 ** rs.uniform(-2.9, 1, k)
    if k:
        ye[pos[0]] = 10.0
    ye[at] = 1e-3
    return ye


@pytest.mark.parametrize("n", N_LONG)
def test_nocorr_and_scaled_error_laws(engine, n):
    """The nocorr law, and the scaled-error law with its minimum error at the first, a middle and the last sample."""
    rs = np.random.RandomState(n + 2)
    yobs = rs.normal(0, 1, n)
    B = 12
    ymod = yobs + np.vstack((residuals(rs, B // 2, n), residuals(rs, B - B // 2, n, smooth=True)))
    noise = np.column_stack((np.zeros(B), rs.uniform(0.01, 0.1, B)))
    descs = [user(E.LAW_NOCORR, n, yobs)]
    engine.set_targets(descs)
    check(engine.loglike_batch(ymod, noise), descs, ymod, noise, "nocorr n=%d" % n)
    for at in sorted({0, n // 2, n - 1}):
        descs = [user(E.LAW_NOCORR_SCALED, n, yobs, yerr=scaled_yerr(rs, n, at))]
        engine.set_targets(descs)
        check(engine.loglike_batch(ymod, noise), descs, ymod, noise, "scaled n=%d min at %d" % (n, at))


@pytest.mark.parametrize("n", [64, 300])
def test_scaled_error_law_overflowing_product(engine, n):
    """Wide error bars over many samples: the reference's np.log(np.product(yerr / yerr.min())) overflows to inf in float64
    and its logL is -inf.  The engine returns what that formula returns: logL = -inf (finite misfits, no failure flag)."""
    rs = np.random.RandomState(n)
    yerr = 10.0 ** rs.uniform(-3, 1, n)
    yerr[0] = 1e-3
    yerr[1] = 10.0
    with np.errstate(over="ignore"):
        overflows = np.isinf(np.prod(yerr / yerr.min()))
    assert overflows == (n == 300)
    yobs = rs.normal(0, 1, n)
    ymod = yobs + residuals(rs, 5, n)
    noise = np.column_stack((np.zeros(5), rs.uniform(0.01, 0.1, 5)))
    descs = [user(E.LAW_NOCORR_SCALED, n, yobs, yerr=yerr)]
    engine.set_targets(descs)
    got = engine.loglike_batch(ymod, noise)
    check(got, descs, ymod, noise, "scaled n=%d, overflowing product" % n)
    assert np.all(got[0] == -np.inf) == overflows


def mixed_targets(rs, ns_laws):
    descs = []
    for n, law in ns_laws:
        yobs = rs.normal(0, 1, n)
        kw = {}
        if law == E.LAW_NOCORR_SCALED:
            kw["yerr"] = scaled_yerr(rs, n, n // 2)
        if law == E.LAW_GAUSS:
            kw["rinv"], kw["logdet_r"] = gauss_matrix("pinv" if n % 2 else "random", n)
        descs.append(user(law, n, yobs, **kw))
    return descs


def mixed_batch(rs, descs, B):
    ymod = np.hstack([d["yobs"] + residuals(rs, B, d["n"], smooth=bool(i % 2)) for i, d in enumerate(descs)])
    noise = np.zeros((B, 2 * len(descs)))
    for t, d in enumerate(descs):
        if d["law"] == E.LAW_EXP:
            noise[:, 2 * t] = rs.choice(R_SET, B)
        elif d["law"] == E.LAW_GAUSS:
            noise[:, 2 * t] = 0.92
        noise[:, 2 * t + 1] = rs.uniform(0.01, 0.1, B)
    return ymod, noise


SMALL = [(30, E.LAW_NOCORR), (64, E.LAW_EXP), (17, E.LAW_NOCORR_SCALED), (40, E.LAW_GAUSS), (1, E.LAW_EXP)]
SHORT_LONG = [(30, E.LAW_EXP), (1000, E.LAW_EXP), (5, E.LAW_NOCORR_SCALED)]
EIGHT = [(30, E.LAW_NOCORR), (65, E.LAW_GAUSS), (1, E.LAW_EXP), (200, E.LAW_NOCORR_SCALED), (300, E.LAW_GAUSS),
         (1025, E.LAW_EXP), (1, E.LAW_NOCORR), (64, E.LAW_NOCORR_SCALED)]


@pytest.mark.parametrize("B", [1, 2, 3, 5, 4097])
def test_all_short_targets_like_small_kernel(engine, B):
    """Every target n <= 64 (a Gauss law among them, its sums from the contraction): one wavefront per model, four models per
    workgroup -- B = 1, 2, 3, 5 and 4097 leave the last workgroup partly empty."""
    rs = np.random.RandomState(B)
    descs = mixed_targets(rs, SMALL)
    ymod, noise = mixed_batch(rs, descs, B)
    engine.set_targets(descs)
    check(engine.loglike_batch(ymod, noise), descs, ymod, noise, "small targets B=%d" % B)


@pytest.mark.parametrize("case", ["short_long", "eight"])
def test_like_kernel_short_beside_long_and_eight_targets(engine, case):
    """like_kernel with a short target beside a long one (the wavefront-only reduction of the short ones), and BH_MAX_TARGETS
    = 8 targets mixing all four laws with two Gauss-law targets, each with its own partial-sum buffer."""
    rs = np.random.RandomState(len(case))
    descs = mixed_targets(rs, SHORT_LONG if case == "short_long" else EIGHT)
    ymod, noise = mixed_batch(rs, descs, 300)
    engine.set_targets(descs)
    check(engine.loglike_batch(ymod, noise), descs, ymod, noise, case)


@pytest.mark.parametrize("case", ["small", "eight"])
def test_per_target_failure_flags(engine, case):
    """loglike_batch(fail=...) with flags in the first, a middle and the last target: those models get logL -1e15, all misfits
    1e15 and err 1 (Targets.py:325-328); every other model has the bits of the call without flags, within the bound."""
    rs = np.random.RandomState(5)
    descs = mixed_targets(rs, SMALL if case == "small" else EIGHT)
    nt, B = len(descs), 130
    ymod, noise = mixed_batch(rs, descs, B)
    engine.set_targets(descs)
    clean = engine.loglike_batch(ymod, noise)
    fail = np.zeros((nt, B), dtype=np.int32)
    fail[0, [0, 63]] = 1
    fail[nt // 2, [64, 65, 100]] = 1
    fail[nt - 1, [127, 129]] = 1
    logL, misf, err = engine.loglike_batch(ymod, noise, fail)
    bad = fail.any(axis=0)
    assert np.array_equal(err != 0, bad)
    assert np.all(logL[bad] == -1e15) and np.all(misf[bad] == 1e15)
    assert np.array_equal(logL[~bad], clean[0][~bad]) and np.array_equal(misf[~bad], clean[1][~bad])
    check(clean, descs, ymod, noise, "failure flags, %s" % case)


def _rf_workload(engine):
    import bench
    spec, batches, noise, truth, nrs = bench.build_workload("c3g", 4096, 10, 1234)
    bench.observed_data(engine, spec, truth, nrs)
    return spec, batches[0], noise


def test_c3g_likelihood_of_the_engines_own_synthetics(engine):
    """bench's c3g workload as bench.build_workload builds it (Rayleigh + Love phase velocities, nocorr; P receiver function,
    n = 1024, Gauss law r = 0.92, rcond 1e-6; B = 4096: the 128 x 128 form with K split 2): logL and misfits of
    evaluate_batch against the reference of the synthetics it returns; the call without synthetics has the same bits."""
    spec, (nlay, h, vp, vs, rho), noise = _rf_workload(engine)
    engine.set_targets(spec)
    logL, misf, err, ymod = engine.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True)
    L2, m2, e2 = engine.evaluate_batch(nlay, h, vp, vs, noise, rho=rho)
    assert np.array_equal(err, e2) and np.array_equal(logL, L2) and np.array_equal(misf, m2)
    ok = err == 0
    assert ok.mean() > 0.9 and np.all(logL[~ok] == -1e15)
    check((logL[ok], misf[ok], err[ok]), spec, ymod[ok], noise[ok], "c3g")


@pytest.mark.parametrize("n,nsamp,fsamp,B", [(1024, 2048, 20.0, 96), (16385, 32768, 100.0, 24)])
def test_fused_exponential_receiver_function_against_the_reference(engine, n, nsamp, fsamp, B):
    """Exponential law on a receiver function, r up to +-0.9999: the fused call (the synthesis kernel forms the sums; at
    n = 16385 from the HBM workspace) and the call that returns the trace give the same bits, and that logL is within the bound
    of the reference of the returned trace -- so an error shared by the fused and the unfused sums is caught too."""
    from bayhunter_amd.synth import synth_models
    rs = np.random.RandomState(n)
    nlay, h, vp, vs, rho = synth_models(rs, B, 10, ragged=True)
    per = np.linspace(2, 40, 20)
    t = np.arange(n) / fsamp
    descs = [{"kind": E.TARGET_SWD, "law": E.LAW_NOCORR, "n": per.size, "x": per, "yobs": 3.4 + 0.01 * per, "iwave": 2, "igr": 0},
             {"kind": E.TARGET_RF, "law": E.LAW_EXP, "n": n, "yobs": 0.01 * np.sin(0.7 * t), "waveno": 0, "nsamp": nsamp,
              "p": 6.4, "gauss": 2.0, "fsamp": fsamp, "tshift": 5.0}]
    engine.set_targets(descs)
    noise = np.column_stack([np.zeros(B), rs.uniform(0.01, 0.05, B), np.resize(np.array(R_SET), B), rs.uniform(0.005, 0.05, B)])
    L1, m1, e1 = engine.evaluate_batch(nlay, h, vp, vs, noise, rho=rho)
    L2, m2, e2, y2 = engine.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True)
    assert np.array_equal(e1, e2) and np.array_equal(L1, L2) and np.array_equal(m1, m2)
    ok = e1 == 0
    assert ok.mean() > 0.8
    check((L1[ok], m1[ok], e1[ok]), descs, y2[ok], noise[ok], "fused RF exp n=%d" % n)


# ---- the six launch paths of the likelihood, bit for bit against the build before the engine's site state became one SiteTable ----
LAUNCH_PATHS = ("plain", "sites", "x", "missing", "classes", "laws")   # bh_launch_like, _sites, _sites_x, _sites_m, _sites_c, _sites_l
LAUNCH_FORMS = {"small": 3, "workgroup": 65}                           # samples of the receiver function beside a curve of 3 periods


def launch_path_outputs(eng, path, form, B):
    """(logL, misfits, err) of B models over [Rayleigh phase velocities at 3 periods, scaled-error law; P receiver function of 3
    or 65 samples, Gauss law] and three sites, through one launch path.  Site 1 has two periods ("x") or lacks the curve
    ("missing" and up), has the second correlation class ("classes") and the nocorr law on its receiver function ("laws", where
    site 0's curve is under the exponential law); model 3 of 5 names a site out of range (the device entry fails it in band)."""
    from bayhunter_amd.synth import synth_models
    from test_gpu_sites import eval_device
    n = LAUNCH_FORMS[form]
    rs = np.random.RandomState(100 * n + B)
    ldy, per = 3 + n, np.array([5.0, 12.0, 30.0])
    yobs = np.hstack([3.2 + 0.02 * per + rs.normal(0, 0.05, (3, 3)), rs.normal(0, 0.05, (3, n))])
    yerr = rs.uniform(0.02, 0.06, (3, ldy))
    mats = [gauss_matrix(kind, n) for kind in ("pinv", "random")]
    descs = [dict(kind=E.TARGET_SWD, law=E.LAW_NOCORR_SCALED, n=3, x=per, yobs=yobs[0, :3], yerr=yerr[0, :3], iwave=2, igr=0),
             dict(kind=E.TARGET_RF, law=E.LAW_GAUSS, n=n, yobs=yobs[0, 3:], waveno=0, p=6.4, gauss=2.5, tshift=5.0, nsamp=128,
                  fsamp=5.0, rinv=mats[0][0], logdet_r=mats[0][1])]
    nlay, h, vp, vs, rho = synth_models(rs, B, 10, ragged=True)
    noise = np.column_stack([np.zeros(B), rs.uniform(0.02, 0.1, B), np.full(B, 0.92), rs.uniform(0.02, 0.1, B)])
    site = np.array([1] if B == 1 else [0, 1, 2, 3, 1], dtype=np.int32)
    eng.set_targets(descs)
    if path == "plain":
        return eng.evaluate_batch(nlay, h, vp, vs, noise, rho=rho)
    cnt = np.array([[3, n], [2 if path == "x" else 0, n], [1, n]], dtype=np.int32)
    x = np.zeros((3, ldy))
    x[:, :3] = per
    if path == "sites":
        eng.set_sites(yobs, yerr)
    else:
        {"x": eng.set_sites_x, "missing": eng.set_sites_missing}.get(path, eng.set_sites_missing_gauss)(cnt, x, yobs, yerr)
        eng.set_sites_rf(np.tile([0.0, 6.4], (3, 1)), np.zeros((3, 2)))
    if path == "laws":
        eng.set_sites_laws(np.array([[E.LAW_EXP, E.LAW_GAUSS], [0, E.LAW_NOCORR], [E.LAW_NOCORR_SCALED, E.LAW_GAUSS]], dtype=np.int32), yerr)
    if path in ("classes", "laws"):
        eng.set_sites_gauss(1, np.array([0, -1 if path == "laws" else 1, 0], dtype=np.int32), np.stack([m[0] for m in mats]),
                            np.array([m[1] for m in mats]))
    return eval_device(eng, (nlay, h, vp, vs, rho), noise, site, ldy)[:3]


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("form", sorted(LAUNCH_FORMS))
@pytest.mark.parametrize("path", LAUNCH_PATHS)
def test_every_launch_path_keeps_the_recorded_bits(engine, path, form, B):
    """tests/golden/like_paths_golden.npz holds what launch_path_outputs returned on an MI355X from the commit before run_like took
    its launcher, tables and count source from the site plan and the SiteTable (recorded once with that build's library; not
    from the code under test).  It also stands ready for a change of the kernels themselves."""
    from conftest import golden
    want = golden("like_paths_golden.npz")
    got = launch_path_outputs(engine, path, form, B)
    if B == 5 and path != "plain":
        assert got[2][3] == 1 and got[0][3] == -1e15 and np.all(got[1][3] == 1e15), "the model of a site out of range"
        assert np.all(got[2][[0, 1, 2, 4]] == 0)
    if path in ("missing", "classes", "laws"):
        assert got[1][-1, 0] == 0.0, "the misfit of the curve site 1 lacks"
    for name, a in zip(("logL", "misfits", "err"), got):
        w = want["%s_%s_%d_%s" % (path, form, B, name)]
        assert a.dtype == w.dtype and a.shape == w.shape and a.tobytes() == w.tobytes(), "%s %s B=%d: %s" % (path, form, B, name)
