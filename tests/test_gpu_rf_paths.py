"""Every launch path of the receiver function (bh_launch_rf) against the extended-precision reference (tests/rf_ref.py):
each trace within FACTOR x its a priori bound, NaN rows where the reference has them; switches that choose between equivalent
code paths give the default's bits.  Also the synthesis kernel's own elementary functions (bh_probe_math ops 11-16)."""
import mpmath
import numpy as np
import pytest

import rf_ref as RR
from bayhunter_amd import engine as E
from bayhunter_amd.synth import prior_models, synth_models

pytestmark = pytest.mark.gpu
LD = np.longdouble


def _check(rf, ref, what):
    worst, ill = RR.check(rf, ref, "bound", what=what)
    print("%s: error / bound %.3e, %d ill samples skipped" % (what, worst, ill))
    return worst


def _cmp(engine, args, what, **kw):
    rf = engine.rf_batch(*args, **kw)
    _check(rf, RR.rf_ref(*args, **kw), what)
    return rf


@pytest.fixture
def tuned(engine):
    """engine.set_tuning(name, value) for one test; every switch it touched is restored."""
    saved = {}

    def set_(name, value):
        saved.setdefault(name, engine.tuning(name))
        engine.set_tuning(name, value)
    yield set_
    for k, v in saved.items():
        engine.set_tuning(k, v)


# ---- elementary functions ---------------------------------------------------------------------------------------------------
def _mp(f, x):
    with mpmath.workdps(40):
        return np.array([float(f(mpmath.mpf(float(v)))) for v in x])


def test_probe_rcp_rsq(engine):
    rs = np.random.RandomState(1)
    x = np.concatenate([10.0 ** rs.uniform(-30, 30, 4000), -10.0 ** rs.uniform(-12, 12, 500), [1.0, 2.0, 0.5, 3.0]])
    got = engine.probe_math(11, x)
    rrel = np.abs((got.astype(LD) - 1 / x.astype(LD)) * x.astype(LD)).astype(float)
    assert rrel.max() <= RR.EPS_KERNEL["rcp"], rrel.max()
    xp = np.abs(x)
    got = engine.probe_math(12, xp)
    want = 1 / np.sqrt(xp.astype(LD))
    rel = np.abs((got.astype(LD) - want) / want).astype(float)
    assert rel.max() <= RR.EPS_KERNEL["rsq"], rel.max()
    print("rcp_nr %.3e, rsq_nr %.3e (eps %.3e)" % (rrel.max(), rel.max(), RR.EPS_KERNEL["rcp"]))


def test_probe_sincos(engine):
    rs = np.random.RandomState(2)
    x = np.concatenate([rs.uniform(-10, 10, 2000), rs.uniform(-RR.SIN_RANGE, RR.SIN_RANGE, 2000),
                        np.pi / 2 * np.arange(-40, 41), [0.0, -0.0, 1e-300, RR.SIN_RANGE - 0.5]])
    for op, f in ((13, mpmath.sin), (14, mpmath.cos)):
        err = np.abs(engine.probe_math(op, x) - _mp(f, x))
        assert err.max() <= RR.EPS_KERNEL["sin"], (op, err.max())
    # past the documented range: the reduction keeps working while k fits an int (|x| < 2^31 pi / 2); report how far it is good
    big = rs.uniform(RR.SIN_RANGE, 2.0 ** 30, 500)
    eb = max(np.abs(engine.probe_math(13, big) - _mp(mpmath.sin, big)).max(),
             np.abs(engine.probe_math(14, big) - _mp(mpmath.cos, big)).max())
    print("sincos_cw beyond 2^20 (to 2^30): absolute error %.3e (eps_sin %.3e)" % (eb, RR.EPS_KERNEL["sin"]))
    assert eb <= 1e-9


def test_probe_exp(engine):
    rs = np.random.RandomState(3)
    x = np.concatenate([rs.uniform(-700, 700, 3000), rs.uniform(-3, 3, 1000), [0.0, -745.0, 709.5]])
    want = _mp(mpmath.exp, x)
    got = engine.probe_math(15, x)
    ok = want > 2.2250738585072014e-308                      # normal results
    assert np.max(np.abs(got[ok] - want[ok]) / want[ok]) <= RR.EPS_KERNEL["exp"]
    edge = np.array([-800.0, -801.0, -1e6, -np.inf, 800.0, 801.0, 1e6, np.inf, 710.0, -746.0, np.nan])
    g = engine.probe_math(15, edge)
    assert np.all(g[:4] == 0.0) and np.all(g[4:8] == np.inf) and g[8] == np.inf and g[9] == 0.0 and np.isnan(g[10]), g


def test_probe_csqrt(engine):
    rs = np.random.RandomState(4)
    m = 10.0 ** rs.uniform(-6, 3, 3000)
    th = rs.uniform(-np.pi, np.pi, 3000)
    z = m * np.exp(1j * th)
    z = np.concatenate([z, [-4 + 0j, complex(-4, -0.0), 4 + 0j, 0j, 1e-3j, -1e-3j, complex(0.0, -0.0)]])
    pairs = np.stack([z.real, z.imag], axis=1).ravel()
    got = engine.probe_math(16, pairs).reshape(-1, 2)
    want = np.sqrt(z.astype(np.clongdouble))
    a = np.abs(want)
    nz = a > 0
    err = (np.abs(got[:, 0] + 1j * got[:, 1] - want.astype(complex))[nz] / a[nz]).astype(float)
    assert err.max() <= 2 * RR.EPS_KERNEL["rsq"] + 5 * RR.U, err.max()
    assert got[-7, 1] > 0 and got[-6, 1] < 0          # -4 +- 0i: +-2i (the sign of zero picks the side of the cut)
    assert np.all(got[-4] == 0) and np.all(got[-1] == 0)


def test_probe_rejects_unknown_ops(engine):
    for op in (24, -1):                    # (17-23: the dispersion kernels' fast arithmetic, tests/test_gpu_swd_fa.py)
        with pytest.raises(E.EngineError):
            engine.probe_math(op, np.ones(4))


# ---- coefficient paths --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lmax", [1, 2, 16, 17, 32, 33, 64, 100])
@pytest.mark.parametrize("waveno", [0, 1])
def test_coefficient_paths(engine, Lmax, waveno):
    """Lmax <= 16 / <= 32: rf_coef_layers_kernel<16 / 32>; above: the serial rf_coef_kernel.  nlay = 1: the NaN row the kernel
    documents (the reference project reads uninitialised memory there: not compared with the oracle)."""
    rs = np.random.RandomState(10 * Lmax + waveno)
    if Lmax == 1:
        nlay, h, vp, vs, rho = np.ones(3, np.int32), np.zeros((1, 3)), np.full((1, 3), 6.0), np.full((1, 3), 3.5), np.full((1, 3), 2.7)
    else:
        nlay, h, vp, vs, rho = (prior_models if Lmax % 2 else synth_models)(rs, 6, Lmax)
        nlay[0] = Lmax
    args = (nlay, h, vp, vs, rho, 6.4, 2.5, 512, 5.0, 5.0, waveno, 201)
    rf = _cmp(engine, args, "Lmax %d" % Lmax)
    if Lmax == 1:
        assert np.all(np.isnan(rf))


def test_ragged_batch_deep_arrays(engine):
    rs = np.random.RandomState(5)
    nlay, h, vp, vs, rho = synth_models(rs, 40, 100, ragged=True)
    nlay[:] = np.minimum(nlay, rs.randint(2, 8, 40))           # Lmax >> nlay
    _cmp(engine, (nlay, h, vp, vs, rho, 6.4, 2.5, 256, 5.0, 5.0, 0, 256), "ragged Lmax 100")


def test_same_models_same_bits_at_every_array_depth(engine):
    """The same 2..12-layer models in arrays of 12, 20 and 40 layers (rf_coef_layers_kernel<16>, <32>, rf_coef_kernel)."""
    rs = np.random.RandomState(6)
    nlay, h, vp, vs, rho = synth_models(rs, 24, 12, lvz_frac=0.3, ragged=True)
    out = []
    for L in (12, 20, 40):
        pad = lambda a: np.vstack([a, np.full((L - 12, a.shape[1]), 7.7)])
        for waveno in (0, 1):
            out.append(engine.rf_batch(nlay, pad(h), pad(vp), pad(vs), pad(rho), 6.4, 2.5, 1024, 10.0, 5.0, waveno, 512))
    for k in (2, 4):
        assert np.array_equal(out[0].view(np.int64), out[k].view(np.int64))
        assert np.array_equal(out[1].view(np.int64), out[k + 1].view(np.int64))


@pytest.mark.parametrize("Lmax", [8, 24, 40])
def test_nonfinite_inputs_in_each_path(engine, Lmax):
    rs = np.random.RandomState(Lmax)
    nlay, h, vp, vs, rho = synth_models(rs, 8, Lmax)
    vp[2, 1] = np.inf
    rho[3, 3] = np.nan
    vs[1, 5] = 0.0
    h[0, 6] = np.nan
    rf = _cmp(engine, (nlay, h, vp, vs, rho, 6.4, 2.5, 512, 5.0, 5.0, 0, 201), "non-finite Lmax %d" % Lmax)
    assert np.all(~np.isfinite(rf).all(axis=1)[[1, 3, 5, 6]])


# ---- synthesis variants ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch,value", [("rf_threads", 128), ("rf_waves", 3), ("rf_no_rot", 1)])
def test_synthesis_variants_same_bits(engine, tuned, switch, value):
    rs = np.random.RandomState(7)
    nlay, h, vp, vs, rho = prior_models(rs, 50, 14)
    for nsamp, fsamp, nkeep, waveno in ((2048, 20.0, 1024, 0), (512, 5.0, 201, 1), (64, 2.0, 64, 0)):
        args = (nlay, h, vp, vs, rho, 6.4, 2.5, nsamp, fsamp, 5.0, waveno, nkeep)
        base = engine.rf_batch(*args)
        tuned(switch, value)
        alt = engine.rf_batch(*args)
        tuned(switch, 0)
        assert np.array_equal(base.view(np.int64), alt.view(np.int64)), (switch, nsamp)
    _check(alt, RR.rf_ref(*args), switch)


@pytest.mark.parametrize("nsamp,fsamp,nkeep", [(32768, 100.0, 16001), (262144, 400.0, 3000)])
def test_workspace_path(engine, nsamp, fsamp, nkeep):
    rs = np.random.RandomState(nsamp % 97)
    nlay, h, vp, vs, rho = synth_models(rs, 2, 8)
    _cmp(engine, (nlay, h, vp, vs, rho, 6.4, 2.5, nsamp, fsamp, 5.0, 1, nkeep), "nsamp %d" % nsamp)


# ---- joint calls --------------------------------------------------------------------------------------------------------------
def _joint(engine, Lmax, rf_targets, B=40):
    rs = np.random.RandomState(Lmax)
    nlay, h, vp, vs, rho = synth_models(rs, B, Lmax, ragged=True)
    per = np.linspace(3, 40, 12)
    descs = [{"kind": E.TARGET_SWD, "law": E.LAW_NOCORR, "n": 12, "x": per, "yobs": 3.5 + 0 * per, "iwave": 2, "igr": 0}]
    for (waveno, nsamp, fsamp, n) in rf_targets:
        descs.append({"kind": E.TARGET_RF, "law": E.LAW_EXP, "n": n, "yobs": np.zeros(n), "waveno": waveno, "nsamp": nsamp,
                      "p": 6.4, "gauss": 2.5, "fsamp": fsamp, "tshift": 5.0})
    engine.set_targets(descs)
    noise = np.tile(np.array([0.0, 0.05] + [0.4, 0.05] * len(rf_targets)), (B, 1))
    rho = 0.32 * vp + 0.77
    ymod = engine.evaluate_batch(nlay, h, vp, vs, noise, rho=rho, want_ymod=True)[3]
    out, off = [], 12
    for (waveno, nsamp, fsamp, n) in rf_targets:
        args = (nlay, h, vp, vs, rho, 6.4, 2.5, nsamp, fsamp, 5.0, waveno, n)
        out.append((ymod[:, off:off + n], args))
        off += n
    return out


@pytest.mark.parametrize("Lmax", [12, 24, 40])
@pytest.mark.parametrize("schedule", ["gated", "rf_coef_big", "rf_keep_floor"])
def test_joint_call_rf_slice(engine, tuned, Lmax, schedule):
    """Gated (rf_coef_layers_kernel_small<16 / 32> at Lmax 12 / 24), the large-register build beside the dispersion kernel,
    the ungated schedule: the RF slice of evaluate_batch is rf_batch's bits and within the bound."""
    if schedule != "gated":
        tuned(schedule, 1)
    for got, args in _joint(engine, Lmax, [(0, 512, 5.0, 201)]):
        assert np.array_equal(got.view(np.int64), engine.rf_batch(*args).view(np.int64))
        _check(got, RR.rf_ref(*args), "joint %s Lmax %d" % (schedule, Lmax))


def test_joint_call_without_overlap(engine):
    """no_overlap is read when an engine is created: a fresh engine with it set, the setting restored afterwards."""
    before = engine.tuning("no_overlap")
    engine.set_tuning("no_overlap", 1)
    try:
        eng = E.Engine(0)
        for got, args in _joint(eng, 24, [(0, 512, 5.0, 201), (1, 1024, 10.0, 300)]):
            assert np.array_equal(got.view(np.int64), eng.rf_batch(*args).view(np.int64))
            _check(got, RR.rf_ref(*args), "joint no_overlap")
        eng.close()
    finally:
        engine.set_tuning("no_overlap", before)


def test_joint_call_two_workspaces(engine):
    """A P target of 2048 samples (LDS) and an SV target of 32768 (HBM workspace) in one call."""
    for got, args in _joint(engine, 10, [(0, 2048, 20.0, 1024), (1, 32768, 100.0, 2001)], B=6):
        assert np.array_equal(got.view(np.int64), engine.rf_batch(*args).view(np.int64))
        _check(got, RR.rf_ref(*args), "joint nsamp %d" % args[7])


# ---- spectrum and outputs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsamp,fsamp,gauss", [(64, 20.0, 0.1), (64, 2.0, 2.5), (256, 5.0, 10.0), (512, 5.0, 5.0)])
def test_cutoff_regimes(engine, nsamp, fsamp, gauss):
    """jcut = 1 (only the DC bin), jcut at and past N/2 (the Nyquist bin computed), an ordinary cut."""
    jc = RR.jcut_of(nsamp, fsamp, gauss)
    rs = np.random.RandomState(nsamp)
    nlay, h, vp, vs, rho = synth_models(rs, 12, 8, ragged=True)
    _cmp(engine, (nlay, h, vp, vs, rho, 6.4, gauss, nsamp, fsamp, 5.0, 0, nsamp), "jcut %d of %d" % (jc, nsamp // 2))


def test_cutoff_regimes_cover_the_edges():
    assert RR.jcut_of(64, 20.0, 0.1) == 1
    assert RR.jcut_of(64, 2.0, 2.5) == 33 and RR.jcut_of(256, 5.0, 10.0) == 129


@pytest.mark.parametrize("nkeep", [0, 1, 2, 77, 256])
def test_nkeep(engine, nkeep):
    rs = np.random.RandomState(nkeep)
    nlay, h, vp, vs, rho = synth_models(rs, 9, 6)
    rf = _cmp(engine, (nlay, h, vp, vs, rho, 6.4, 2.5, 256, 5.0, 5.0, 1, nkeep), "nkeep %d" % nkeep)
    assert rf.shape == (9, nkeep)


@pytest.mark.parametrize("tshift", [0.0, -7.5, 60.0, 5000.0, 2.0e5])
def test_time_shift(engine, tshift):
    """tshift 0, negative, beyond N / fsamp (51.2 s), and large |w tshift| (up to 2e5 s x pi 5 Hz: 3e6 rad, past 2^20)"""
    rs = np.random.RandomState(11)
    nlay, h, vp, vs, rho = synth_models(rs, 9, 6)
    _cmp(engine, (nlay, h, vp, vs, rho, 6.4, 2.5, 256, 5.0, tshift, 0, 256), "tshift %g" % tshift)


def test_model_major_layout_and_device_strides(engine):
    import torch
    rs = np.random.RandomState(12)
    nlay, h, vp, vs, rho = synth_models(rs, 16, 10, ragged=True)
    args = (nlay, h, vp, vs, rho, 6.4, 2.5, 512, 5.0, 5.0, 0, 201)
    lm = _cmp(engine, args, "layer_major")
    mm = engine.rf_batch(nlay, h.T.copy(), vp.T.copy(), vs.T.copy(), rho.T.copy(), 6.4, 2.5, 512, 5.0, 5.0, 0, 201,
                         layout="model_major")
    assert np.array_equal(lm.view(np.int64), mm.view(np.int64))
    # device call, model-major rows of sb = 13 > Lmax = 10 doubles
    dev = torch.device("cuda:0")
    pad = lambda a: torch.tensor(np.hstack([a.T, np.full((16, 3), np.nan)]), dtype=torch.float64, device=dev).contiguous()
    th, tvp, tvs, trho = pad(h), pad(vp), pad(vs), pad(rho)
    tn = torch.tensor(nlay, dtype=torch.int32, device=dev)
    out = torch.zeros((16, 201), dtype=torch.float64, device=dev)
    engine.rf_batch_dev(16, 10, tn.data_ptr(), th.data_ptr(), tvp.data_ptr(), tvs.data_ptr(), trho.data_ptr(), 1, 13, 6.4, 2.5,
                        512, 5.0, 5.0, 0, 201, out.data_ptr(), stream=None)
    engine.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.int64), lm.view(np.int64))
