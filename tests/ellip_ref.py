"""Rayleigh ellipticity, restated twice without the library.

1. `ellip`, `ellip_batch`: include/bh_engine_swd_ellip.h in plain Python floats -- the model rounded to binary32, the host libm's
   sincos and exp, the reference's operation order, the secant polish.  The kernel (bayhunter_amd/csrc/swd_ellip.hip) returns
   these bits.  (sincos through ctypes, not math.sin and math.cos: the compiled reference calls sincos, which is what
   bh_libm.h restates, and glibc's sin / cos differ from it in the last bit for about one argument in a thousand.)
2. `ode_ratios`: an independent route.  The motion-stress vector r = (r1, r2, r3, r4) of Aki & Richards (7.28), dr/dz = A r with
   u_x = r1 e^{i(kx - wt)}, u_z = i r2 e^{i(kx - wt)}, z downward; the two solutions that decay in the half-space are carried up
   to the free surface through the layers' matrix exponentials (a Taylor series with scaling and squaring, all in numpy
   longdouble), and the surface u_x / u_z of the combination with vanishing traction is a ratio of 2x2 minors of the two
   solutions: m(0,2) / m(1,2) from the r3 row, m(0,3) / m(1,3) from the r4 row.  Its sign convention is the opposite one (positive
   = prograde).  Thomson-Haskell propagation loses what the growing exponentials swallow: the two ratios drift apart where it
   breaks down, which is how a test knows where it can be trusted.
"""
import ctypes
import ctypes.util
import math

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.sincos.argtypes = [ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
_libm.sincos.restype = None
_sn, _cs = ctypes.c_double(), ctypes.c_double()


def _sincos(x):
    _libm.sincos(x, ctypes.byref(_sn), ctypes.byref(_cs))
    return _sn.value, _cs.value


TWOPI = 2.0 * 3.141592653589793
NAN = float("nan")
MISMATCH_MAX = 1.0e-2   # BH_ELLIP_MISMATCH_MAX: an entry whose mismatch is not at most this raises the flag


def f32(x):
    return float(np.float32(x))


def _fmax(a, b):   # C's fmax: a NaN operand is ignored
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def _div(a, b):    # IEEE division where Python raises
    try:
        return a / b
    except ZeroDivisionError:
        if a == 0.0 or a != a:
            return NAN
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _exp_m2(p):
    return math.exp(-2.0 * p) if p < 16.0 else 0.0


def _layer_products(p, q, ra, rb, wvno, xka, xkb, dpth):
    """surfdisp96.f:874-991 (`var`) as swd_common.h's layer_products computes it."""
    pex = sex = 0.0
    if wvno < xka:
        sinp, cosp = _sincos(p)
        w = sinp / ra
        x = -ra * sinp
    elif wvno == xka:
        cosp, w, x = 1.0, dpth, 0.0
    else:
        pex = p
        fac = _exp_m2(p)
        cosp = (1.0 + fac) * 0.5
        sinp = (1.0 - fac) * 0.5
        w = sinp / ra
        x = ra * sinp
    if wvno < xkb:
        sinq, cosq = _sincos(q)
        y = sinq / rb
        z = -rb * sinq
    elif wvno == xkb:
        cosq, y, z = 1.0, dpth, 0.0
    else:
        sex = q
        fac = _exp_m2(q)
        cosq = (1.0 + fac) * 0.5
        sinq = (1.0 - fac) * 0.5
        y = sinq / rb
        z = rb * sinq
    exa = pex + sex
    a0 = math.exp(-exa) if exa < 60.0 else 0.0
    return (a0, cosp * cosq, cosp * y, cosp * z, cosq * w, cosq * x, x * y, x * z, w * y, w * z)


def _apply_layer(e, wvno2, gam, gammk, rho, v):
    """surfdisp96.f:1024-1068 (`dnka`), e <- e * CA (:836-842), normc (:995-1020)."""
    a0, cpcq, cpy, cpz, cqw, cqx, xy, xz, wy, wz = v
    two = 2.0
    gamm1 = gam - 1.0
    twgm1 = gam + gamm1
    gmgmk = gam * gammk
    gmgm1 = gam * gamm1
    gm1sq = gamm1 * gamm1
    rho2 = rho * rho
    a0pq = a0 - cpcq
    ca11 = cpcq - two * gmgm1 * a0pq - gmgmk * xz - wvno2 * gm1sq * wy
    ca12 = (wvno2 * cpy - cqx) / rho
    ca13 = -(twgm1 * a0pq + gammk * xz + wvno2 * gamm1 * wy) / rho
    ca14 = (cpz - wvno2 * cqw) / rho
    ca15 = -(two * wvno2 * a0pq + xz + wvno2 * wvno2 * wy) / rho2
    ca21 = (gmgmk * cpz - gm1sq * cqw) * rho
    ca22 = cpcq
    ca23 = gammk * cpz - gamm1 * cqw
    ca24 = -wz
    ca41 = (gm1sq * cpy - gmgmk * cqx) * rho
    ca42 = -xy
    ca43 = gamm1 * cpy - gammk * cqx
    ca51 = -(two * gmgmk * gm1sq * a0pq + gmgmk * gmgmk * xz + gm1sq * gm1sq * wy) * rho2
    ca53 = -(gammk * gamm1 * twgm1 * a0pq + gam * gammk * gammk * xz + gamm1 * gm1sq * wy) * rho
    t = -two * wvno2
    ca31 = t * ca53
    ca32 = t * ca43
    ca33 = a0 + two * (cpcq - ca11)
    ca34 = t * ca23
    ca35 = t * ca13
    ca25, ca44, ca45, ca52, ca54, ca55 = ca14, ca22, ca12, ca41, ca21, ca11
    e0, e1, e2, e3, e4 = e
    ee0 = 0.0 + e0 * ca11; ee0 = ee0 + e1 * ca21; ee0 = ee0 + e2 * ca31; ee0 = ee0 + e3 * ca41; ee0 = ee0 + e4 * ca51
    ee1 = 0.0 + e0 * ca12; ee1 = ee1 + e1 * ca22; ee1 = ee1 + e2 * ca32; ee1 = ee1 + e3 * ca42; ee1 = ee1 + e4 * ca52
    ee2 = 0.0 + e0 * ca13; ee2 = ee2 + e1 * ca23; ee2 = ee2 + e2 * ca33; ee2 = ee2 + e3 * ca43; ee2 = ee2 + e4 * ca53
    ee3 = 0.0 + e0 * ca14; ee3 = ee3 + e1 * ca24; ee3 = ee3 + e2 * ca34; ee3 = ee3 + e3 * ca44; ee3 = ee3 + e4 * ca54
    ee4 = 0.0 + e0 * ca15; ee4 = ee4 + e1 * ca25; ee4 = ee4 + e2 * ca35; ee4 = ee4 + e3 * ca45; ee4 = ee4 + e4 * ca55
    t1 = _fmax(_fmax(_fmax(abs(ee0), abs(ee1)), _fmax(abs(ee2), abs(ee3))), abs(ee4))
    if t1 < 1.0e-40:
        t1 = 1.0
    return [ee0 / t1, ee1 / t1, ee2 / t1, ee3 / t1, ee4 / t1]


def round_model(h, vp, vs, rho):
    """the layers as the kernels see them: binary32 values as Python floats"""
    return [[f32(v) for v in a] for a in (h, vp, vs, rho)]


def vector(model, T, c):
    """E(c) and k of the header; model = round_model(...) of one model's own layers (the last is the half-space)."""
    d, a, b, r = model
    mmax = len(b)
    omega = TWOPI / T
    wvno = omega / c
    om = 1.0e-4 if omega < 1.0e-4 else omega
    wvno2 = wvno * wvno

    def terms(m):
        xka = om / a[m]
        xkb = om / b[m]
        ra = math.sqrt((wvno + xka) * abs(wvno - xka))
        rb = math.sqrt((wvno + xkb) * abs(wvno - xkb))
        t = b[m] / om
        gammk = 2.0 * t * t
        gam = gammk * wvno2
        return xka, xkb, ra, rb, gammk, gam

    xka, xkb, ra, rb, gammk, gam = terms(mmax - 1)
    gamm1 = gam - 1.0
    rho1 = r[mmax - 1]
    e = [rho1 * rho1 * (gamm1 * gamm1 - gam * gammk * ra * rb), -rho1 * ra, rho1 * (gamm1 - gammk * ra * rb), rho1 * rb,
         wvno2 - ra * rb]
    for m in range(mmax - 2, -1, -1):
        xka, xkb, ra, rb, gammk, gam = terms(m)
        dpth = d[m]
        v = _layer_products(ra * dpth, rb * dpth, ra, rb, wvno, xka, xkb, dpth)
        e = _apply_layer(e, wvno2, gam, gammk, r[m], v)
    return e, wvno


def e0(model, T, c):
    return vector(model, T, c)[0][0]


def ratios(e, k):
    """(hv, hv_alt, mismatch, bad)"""
    if e[1] == 0.0 or e[2] == 0.0:
        return NAN, NAN, NAN, True
    hv = _div(e[3], k * e[2])
    hv_alt = _div(-k * e[2], e[1])
    mis = _div(abs(hv - hv_alt), abs(hv))
    if not (math.isfinite(hv) and math.isfinite(hv_alt) and math.isfinite(mis)):
        return NAN, NAN, NAN, True
    return hv, hv_alt, mis, False


def ellip(model, T, c, nsteps=2, mismatch_max=MISMATCH_MAX):
    """One (model, period) of a model that has a root: (hv, mismatch, cpol, flag) -- the header's polish, results and gate
    (mismatch_max = inf: the call before it had the gate)."""
    if not (model[2][0] > 0.0):     # a water layer
        return NAN, NAN, c, 1
    flag = 0
    if nsteps == 0:
        cpol = c
        e, k = vector(model, T, c)
    else:
        c0 = c
        c1 = c0 * (1.0 + 2.0 ** -20)
        f0 = vector(model, T, c0)[0][0]
        e, k = vector(model, T, c1)
        f1 = e[0]
        cpol = c1
        for _ in range(nsteps):
            if f1 == f0:
                break
            c2 = c1 - f1 * (c1 - c0) / (f1 - f0)
            if not (abs(c2 - c) <= 1.0e-5 * c):
                e, k = vector(model, T, c)
                cpol = c
                flag = 1
                break
            c0, f0 = c1, f1
            c1 = c2
            e, k = vector(model, T, c1)
            f1 = e[0]
            cpol = c1
    hv, hv_alt, mis, bad = ratios(e, k)
    if bad or not (mis <= mismatch_max):   # the gate on the certificate: hv, mis and cpol stay as they are
        flag = 1
    return hv, mis, cpol, flag


def ellip_batch(nlay, h, vp, vs, rho, periods, vel, err, nsteps=2):
    """The call: h, vp, vs, rho [Lmax, B] (layer-major), vel [B, K], err [B] -> hv, mismatch, cpol [B, K], flag [B]."""
    h, vp, vs, rho = [np.asarray(a, dtype=float) for a in (h, vp, vs, rho)]
    vel = np.asarray(vel, dtype=float)
    B, K = vel.shape
    hv, mis, cpol = np.zeros((B, K)), np.zeros((B, K)), np.zeros((B, K))
    flag = np.zeros(B, dtype=np.int32)
    for b in range(B):
        n = int(nlay[b])
        if err[b] != 0 or n < 1 or n > h.shape[0]:
            continue
        model = round_model(h[:n, b], vp[:n, b], vs[:n, b], rho[:n, b])
        for k in range(K):
            c = float(vel[b, k])
            if not (c > 0.0):
                continue
            hv[b, k], mis[b, k], cpol[b, k], f = ellip(model, float(periods[k]), c, nsteps)
            flag[b] |= f
    return hv, mis, cpol, flag


def same_bits(a, b):
    """equal bit for bit, a NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan]))


# ---- the fundamental-mode root of the restatement's e0, to the last bit --------------------------------------------------------
def halfspace_x(alpha, beta):
    """c^2 / beta^2 of the Rayleigh wave of a homogeneous half-space: the root in (0, 1) of the Rayleigh function, bisected in
    longdouble."""
    ld = np.longdouble
    g2 = (ld(beta) / ld(alpha)) ** 2

    def rf(x):
        return (ld(2) - x) ** 2 - ld(4) * np.sqrt(ld(1) - x) * np.sqrt(ld(1) - g2 * x)

    lo, hi = ld(0.5), ld(1) - ld(2) ** -40   # rf < 0 below the root, > 0 just below 1
    assert rf(lo) < 0 < rf(hi)
    for _ in range(200):
        mid = (lo + hi) / 2
        if mid == lo or mid == hi:
            break
        if rf(mid) < 0:
            lo = mid
        else:
            hi = mid
    return lo


def halfspace_hv(alpha, beta):
    """the closed form 2 sqrt(1 - x) / (2 - x), x = c^2 / beta^2, in longdouble"""
    x = halfspace_x(alpha, beta)
    return 2 * np.sqrt(1 - x) / (2 - x)


def bisect_root(model, T, lo, hi):
    """[lo, hi] with e0 of opposite signs -> (c, c_next): neighbouring floats across the sign change (c the one with the smaller
    |e0|)"""
    flo, fhi = e0(model, T, lo), e0(model, T, hi)
    assert flo * fhi <= 0.0
    while True:
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        fm = e0(model, T, mid)
        if (fm < 0.0) == (flo < 0.0) and fm != 0.0:
            lo, flo = mid, fm
        else:
            hi, fhi = mid, fm
    return (lo, hi) if abs(flo) <= abs(fhi) else (hi, lo)


def fundamental_roots(model, periods, dc=0.005):
    """The lowest root of e0 at every period (ascending periods), as the reference looks for it: from 0.8 of the slowest half-space
    Rayleigh velocity at the first period, from 1.5 steps below the last root afterwards, upwards in steps of dc to the first
    sign change, which is bisected to the last bit."""
    d, a, b, r = model
    j = min(range(len(b)), key=lambda i: b[i])
    start = 0.8 * b[j] * math.sqrt(float(halfspace_x(a[j], b[j])))
    out = []
    for T in periods:
        c1 = start
        f1 = e0(model, T, c1)
        while True:
            c2 = c1 + dc
            assert c2 < max(b) + dc, "no root below the fastest S velocity"
            f2 = e0(model, T, c2)
            if (f1 < 0.0) != (f2 < 0.0) or f2 == 0.0:
                break
            c1, f1 = c2, f2
        c = bisect_root(model, T, c1, c2)[0]
        out.append(c)
        start = c - 1.5 * dc
    return out


# ---- the independent route -----------------------------------------------------------------------------------------------------
LD = np.longdouble


def _expm_ld(M):
    """exp(M) of a small real matrix in longdouble: Taylor series of M / 2^s, squared s times"""
    nrm = float(np.max(np.sum(np.abs(M), axis=1)))
    s = max(0, int(math.ceil(math.log2(nrm))) + 3) if nrm > 0 else 0
    X = M / LD(2) ** s
    n = M.shape[0]
    term = np.eye(n, dtype=LD)
    out = np.eye(n, dtype=LD)
    for i in range(1, 40):
        term = term @ X / LD(i)
        out = out + term
    for _ in range(s):
        out = out @ out
    return out


def _ode_matrix(k, w, alpha, beta, rho):
    mu = rho * beta * beta
    lam = rho * alpha * alpha - 2 * mu
    l2m = lam + 2 * mu
    zeta = 4 * mu * (lam + mu) / l2m
    z = LD(0)
    return np.array([[z, k, 1 / mu, z],
                     [-k * lam / l2m, z, z, 1 / l2m],
                     [k * k * zeta - w * w * rho, z, z, k * lam / l2m],
                     [z, -w * w * rho, -k, z]], dtype=LD)


def ode_ratios(model, T, c):
    """(m(0,2) / m(1,2), m(0,3) / m(1,3)) at the free surface, longdouble; c < the half-space's S velocity."""
    d, a, b, r = [[LD(v) for v in arr] for arr in model]
    w = LD(TWOPI) / LD(T)
    k = w / LD(c)
    n = len(b)
    # the half-space's two decaying solutions: potentials exp(-nu z) give (r1, r2) = (k, nu_a) for P and (nu_b, k) for SV; the
    # stresses follow from the first two rows of dr/dz = A r with d/dz = -nu
    A = _ode_matrix(k, w, a[n - 1], b[n - 1], r[n - 1])
    mu = r[n - 1] * b[n - 1] ** 2
    l2m = r[n - 1] * a[n - 1] ** 2
    lam = l2m - 2 * mu
    ys = []
    for i, v in enumerate((a[n - 1], b[n - 1])):
        nu = np.sqrt(k * k - (w / v) ** 2)
        r1, r2 = (k, nu) if i == 0 else (nu, k)
        y = np.array([r1, r2, mu * (-nu * r1 - k * r2), l2m * (-nu) * r2 + k * lam * r1], dtype=LD)
        res = A @ y + nu * y   # an eigenvector of eigenvalue -nu
        assert float(np.max(np.abs(res))) <= 1e-15 * float(np.max(np.abs(y))) * float(np.max(np.abs(A))), "half-space eigenvector"
        ys.append(y)
    Y = np.stack(ys, axis=1)   # [4, 2]
    for m in range(n - 2, -1, -1):   # r(top) = exp(-A h) r(bottom)
        Y = _expm_ld(-_ode_matrix(k, w, a[m], b[m], r[m]) * d[m]) @ Y
        Y = Y / np.max(np.abs(Y), axis=0)

    def minor(i, j):
        return Y[i, 0] * Y[j, 1] - Y[i, 1] * Y[j, 0]

    return minor(0, 2) / minor(1, 2), minor(0, 3) / minor(1, 3)


# ---- the four models of the accuracy tests (h, vp, vs, rho; the last layer is the half-space) -----------------------------------
def _stack(h, vs, vpvs=None, vp=None):
    vs = np.asarray(vs, dtype=float)
    vp = vs * vpvs if vp is None else np.asarray(vp, dtype=float)
    return round_model(np.asarray(h, dtype=float), vp, vs, vp * 0.32 + 0.77)


MODELS = {
    # one Poisson solid cut into layers: the ellipticity of a half-space at every period
    "poisson": _stack([2.0, 5.0, 9.0, 0.0], [3.5] * 4, vp=[3.5 * math.sqrt(3.0)] * 4),
    "crust": _stack([3.0, 12.0, 20.0, 0.0], [2.9, 3.5, 3.8, 4.5], 1.73),
    "sediment": _stack([0.5, 9.0, 25.0, 0.0], [0.6, 3.3, 3.8, 4.5], vp=[2.0, 5.8, 6.6, 8.0]),
    "lvz": _stack([4.0, 8.0, 6.0, 17.0, 0.0], [3.2, 3.7, 3.1, 3.9, 4.5], 1.75),
}
PERIODS = [4.0, 8.0, 12.0, 20.0, 30.0, 40.0]
