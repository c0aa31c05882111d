"""Extended-precision reference of the receiver function (bh_rf_batch) with an a priori error bound.

Not a conftest: a plain module the receiver-function tests import, like like_ref.py.

What it computes
----------------
The path bh_rf_batch defines (include/bh_engine.h; restated from oracle/rf_oracle.c and the comments of csrc/rf_kernel.hip),
for one model at a time, every bin k = 0..N/2 of an N-sample trace (no spectral cut-off):

    depths     z_l = the float64 running sum of h in layer order (as the reference forms them); the thickness of a finite
               layer z_{l+1} - z_l, the half-space's -1
    flattening r = 6371 - z, q = 6371 / r: v *= q, rho /= q, h -> 6371 ln(6371 / (6371 - z_bot)) - 6371 ln q
    matrices   the solid-solid interface matrices rd, td, ru, tu, the free surface's ru and the displacement matrix 2h from
               the flattened real velocities; the P/SV rotation from nsv and the top layer's Poisson ratio when p > 1e-4
               s/km and nsv > 0.01
    recursion  per bin, w = k dw: causal-Q complex slownesses, phases e^{-i w d q}, the Mueller top-down recursion
               nb = e nt e, q = (I - rd nb)^-1 tu, g = g e q; cr, cz from 2h g (P: first column, SV: second), rotated, swapped
               for SV
    division   X_k = cr conj(cz) / |cz|^2 * sqrt(pi) fsamp / a * exp(-(min(w/a, 50))^2 / 4 - i w tshift)
    transform  f = irfft(X)[:nkeep] (the imaginary parts of X_0 and X_{N/2} drop out)

Everything after the float64 inputs (and p = p_deg * 0.00899, formed in float64 as every implementation forms it) is done in
np.longdouble / np.clongdouble.  The common phase e^{i w t0} of the reference cancels in cr conj(cz) / |cz|^2 and is left out;
t0 is still formed, because a NaN t0 (a layer post-critical for the direct wave) makes the reference's whole trace NaN.  A model
whose coefficients are not all finite, or with fewer than two layers, gives a NaN row, as the kernel documents.

The bound
---------
A first-order running error analysis carried along with every value (class _T below).  Each computed quantity x^ = x + dx
carries a bound E >= |dx| in absolute terms; u = 2^-53; the arithmetic may contract products into FMAs (which only removes
roundings).  With |.| the modulus:

    a + b        E_a + E_b + u |a + b|
    a * b        |a| E_b + |b| E_a + 3u |a| |b|               (a complex product: each part two products and a sum)
    1 / b        E_b / |b|^2 + (3u + eps_rcp) / |b|           (|b|^2, its reciprocal, two products: crecip_f)
    sqrt(z)      E_z / (2 |sqrt z|) + (2 eps_rsq + 5u) |sqrt z|   (csqrt_f: |z| through rsq_nr, then sqrt(y) through rsq_nr)
    e^z          |e^z| (E_z + eps_exp + 2 eps_sin + 2u)       (exp_cw of Re z, sincos_cw of Im z; E_z covers both parts)
    ln x, sqrt x E_x / |x| + 2u |ln x|,  E_x / (2 |sqrt x|) + u |sqrt x|

eps_rcp / eps_rsq are the relative errors of rcp_nr / rsq_nr, eps_sin the absolute error of sincos_cw on |x| < 2^20, eps_exp
the relative error of exp_cw (EPS_KERNEL; tests/test_gpu_rf_paths.py probes the very functions at these numbers).  The
frequency-independent coefficients are formed with IEEE division and square roots in every implementation (eps = u).
The input arguments of the phase (w, d, the slownesses) carry their own errors through these rules, so |w tshift| and w d
enter as u |w tshift| etc.  With E_k the bound of bin k so obtained (plus 8u |X_k| for the products by common factors: the
reference's e^{i w t0}, the Gauss factor's constant), a sample of the trace satisfies

    |f^_n - f_n| <= (1/N) sum_k w_k (E_k + cut_k) + (log2 N + 4)(4u + eps_tw) (1/N) sum_k w_k |X_k| + ref_k

with w_k = 1 for k = 0 and N/2 and 2 otherwise (each bin enters the real inverse transform once or as a conjugate pair), cut_k
= |X_k| for the bins the kernel does not form (k >= jcut, bh_rf_axis_cut), the second term the transform's own rounding (every
output is a sum over log2 N radix-2 stages of butterflies whose partial sums are bounded by sum |X|, each stage a twiddle
product and an addition: 4u + eps_tw, eps_tw = 4 eps_sin + 3u for the two-table twiddles; + 4 for the real-to-complex fold
and the 1/N) and ref the reference's own error: the same analysis with the long double unit u_ld = 2^-64 in place of every
epsilon -- to first order the bound is linear in the epsilons, so this is (u_ld / u) times the IEEE set's bound without cut.

Two epsilon sets are carried side by side: EPS_KERNEL with the kernel's cut-off gives `bound`; EPS_F64 (correctly rounded
functions, no cut) gives `f64_bound`, the oracle's arithmetic.  The bound is the same for every sample of a trace.

Where the bound breaks down.  A slowness close to a branch point (p near critical: sqrt(z) with z ~ 0) or a |cz| close to 0
makes the first-order terms explode; such models are `ill` (bound above the trace's peak) and the tests report, not assert, them.

Tolerances are FACTOR x bound (FACTOR <= 8), never fitted to what a GPU returns.
"""
import numpy as np

LD, CLD = np.longdouble, np.clongdouble
U = 2.0 ** -53
U_LD = float(np.finfo(LD).eps) / 2.0
PI = 4 * np.arctan(LD(1))
R_EARTH = LD(6371)
RF_CUT_WA = 12.5132                      # csrc/rf_plan.hip: w / a beyond which the Gauss low-pass is below 1e-17
SIN_RANGE = 2.0 ** 20                    # sincos_cw's documented argument range
FACTOR = 4.0                             # tolerance = FACTOR x bound

# The arithmetic's epsilons (relative for rcp / rsq / exp, absolute on [-1, 1] for sin / cos)
EPS_KERNEL = dict(rcp=2.0 ** -45, rsq=2.0 ** -45, sin=4 * U, exp=4 * U)   # rcp_nr / rsq_nr: (2^-23)^2 + rounding
EPS_F64 = dict(rcp=U, rsq=U, sin=U, exp=U)                                 # correctly rounded IEEE functions


def _eps(name):
    return np.array([EPS_KERNEL[name], EPS_F64[name]]).reshape(2, 1)


def _m(x):
    return np.abs(x).astype(np.float64)


class _T(object):
    """A value (long double, real or complex, [nb] bins) and its error bounds [2, nb] (kernel set, IEEE set)."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = v
        e = np.asarray(e, dtype=np.float64)
        self.e = e if e.ndim == 2 else np.broadcast_to(e, (2,) + (np.shape(v) if np.ndim(v) else (1,)))

    def __add__(self, o):
        o = _t(o)
        v = self.v + o.v
        return _T(v, self.e + o.e + U * _m(v))

    __radd__ = __add__

    def __sub__(self, o):
        o = _t(o)
        v = self.v - o.v
        return _T(v, self.e + o.e + U * _m(v))

    def __rsub__(self, o):
        return _t(o) - self

    def __neg__(self):
        return _T(-self.v, self.e)

    def __mul__(self, o):
        o = _t(o)
        a, b = _m(self.v), _m(o.v)
        return _T(self.v * o.v, a * o.e + b * self.e + 3 * U * a * b)

    __rmul__ = __mul__

    def __truediv__(self, o):
        return self * rcp(_t(o), ieee=True)

    def __rtruediv__(self, o):
        return _t(o) * rcp(self, ieee=True)

    def conj(self):
        return _T(np.conj(self.v), self.e)


def _t(x):
    return x if isinstance(x, _T) else _T(np.asarray(x, dtype=CLD if np.iscomplexobj(x) else LD))


def rcp(b, ieee=False):
    """1 / b: crecip_f (rcp_nr) or, ieee, a correctly rounded division."""
    eps = U if ieee else _eps("rcp")
    a = _m(b.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        return _T(1 / b.v, b.e / a ** 2 + (3 * U + eps) / a)


def csqrt(z, ieee=False):
    """principal square root: csqrt_f (rsq_nr) or, ieee, the library's."""
    eps = U if ieee else _eps("rsq")
    v = np.sqrt(np.asarray(z.v, dtype=CLD))
    a = _m(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        return _T(v, z.e / (2 * a) + (2 * eps + 5 * U) * a)


def cexp(z):
    v = np.exp(np.asarray(z.v, dtype=CLD))
    return _T(v, _m(v) * (z.e + _eps("exp") + 2 * _eps("sin") + 2 * U))


def rlog(x):
    v = np.log(x.v)
    return _T(v, x.e / _m(x.v) + 2 * U * _m(v))


def rsqrt(x):
    v = np.sqrt(x.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        return _T(v, x.e / (2 * _m(v)) + U * _m(v))


def _mat_mul(x, y):
    return (x[0] * y[0] + x[1] * y[2], x[0] * y[1] + x[1] * y[3], x[2] * y[0] + x[3] * y[2], x[2] * y[1] + x[3] * y[3])


def _flatten(z, h, vp, vs, rh):
    """model.cpp's flattening, as rf_oracle.c's flatten_layer restates it: (h, vp, vs, rh) flattened."""
    r = _t(R_EARTH) - z
    q = _t(R_EARTH) / r
    zf = R_EARTH * rlog(q)
    vp, vs, rh = vp * q, vs * q, rh / q
    lower_halfspace = not (h.v > 0) and not (vp.v < 1 and rh.v < 0.1)
    if not lower_halfspace:
        h = R_EARTH * rlog(_t(R_EARTH) / (_t(R_EARTH) - (z + h))) - zf
    return h, vp, vs, rh


def _interface(u, vp1, vs1, rho1, vp2, vs2, rho2):
    """Solid-solid interface, P/SV (rf_oracle.c interface_coeffs): rd, td, ru, tu as (c11, c12, c21, c22)."""
    mue1, mue2 = rho1 * vs1 * vs1, rho2 * vs2 * vs2
    c = 2.0 * (mue1 - mue2)
    u2 = u * u
    cu2 = c * u2
    a1 = csqrt(_t(1.0) / (vp1 * vp1) - u2, ieee=True).conj()
    a2 = csqrt(_t(1.0) / (vp2 * vp2) - u2, ieee=True).conj()
    b1 = csqrt(_t(1.0) / (vs1 * vs1) - u2, ieee=True).conj()
    b2 = csqrt(_t(1.0) / (vs2 * vs2) - u2, ieee=True).conj()
    t1, t2, t3 = cu2 - rho1 + rho2, cu2 - rho1, cu2 + rho2
    t4 = t3 * a1 - t2 * a2
    abab = c * c * u2 * a1 * a2 * b1 * b2
    d1 = t1 * t1 * u2 + t2 * t2 * a2 * b2 + rho1 * rho2 * a2 * b1
    d2 = abab + t3 * t3 * a1 * b1 + rho1 * rho2 * a1 * b2
    t5 = rcp(d1 + d2, ieee=True)
    t7 = 2.0 * rho1 * t5
    mix = t1 * t3 + c * t2 * a2 * b2
    rd = ((d2 - d1) * t5, 2.0 * u * b1 * t5 * mix, -2.0 * u * a1 * t5 * mix,
          (d2 - d1 - 2.0 * rho1 * rho2 * (a1 * b2 - a2 * b1)) * t5)
    td = (a1 * t7 * (t3 * b1 - t2 * b2), b1 * t7 * u * (t1 + c * a1 * b2), -(a1 * t7) * u * (t1 + c * a2 * b1), b1 * t7 * t4)
    d1 = t1 * t1 * u2 + t3 * t3 * a1 * b1 + rho1 * rho2 * a1 * b2
    d2 = abab + t2 * t2 * a2 * b2 + rho1 * rho2 * a2 * b1
    t5 = rcp(d1 + d2, ieee=True)
    t7 = 2.0 * rho2 * t5
    mix = t1 * t2 + c * t3 * a1 * b1
    ru = ((d2 - d1) * t5, -2.0 * u * b2 * t5 * mix, 2.0 * u * a2 * t5 * mix,
          (d2 - d1 - 2.0 * rho1 * rho2 * (a2 * b1 - a1 * b2)) * t5)
    tu = (a2 * t7 * (t3 * b1 - t2 * b2), b2 * t7 * u * (t1 + c * a2 * b1), -(a2 * t7) * u * (t1 + c * a1 * b2), b2 * t7 * t4)
    return rd, td, ru, tu


def _free_surface(p, vp, vs):
    """free-surface ru and the displacement matrix times 2 (rf_oracle.c surface_coeffs, displacement_matrix)"""
    p2 = p * p
    a = csqrt(_t(1.0) / (vp * vp) - p2, ieee=True)
    b = csqrt(_t(1.0) / (vs * vs) - p2, ieee=True)
    t1 = 2.0 * vs * vs
    t2 = t1 * p2 - 1.0
    d1 = t2 * t2
    d2 = t1 * t1 * p2 * a * b
    d = d1 + d2
    t3 = 2.0 * t1 * p * t2 / d
    rpp = (d2 - d1) / d
    ru = (rpp, -(b * t3), a * t3, rpp)
    vs2 = vs * vs
    x = 1.0 - 2.0 * vs2 * p2
    a1, b1 = a.conj(), b.conj()
    qq = rcp(x * x + 4.0 * vs2 * vs2 * p2 * a1 * b1, ieee=True)
    hm = (2.0 * (qq * a1 * b1 * (2.0 * vs2 * p)), 2.0 * (qq * b1 * (1.0 - 2.0 * vs2 * p2)),
          2.0 * (qq * a1 * (1.0 - 2.0 * vs2 * p2)), -(2.0 * (qq * a1 * b1 * (2.0 * vs2 * p))))
    return ru, hm


def _finite(*mats):
    return all(np.all(np.isfinite(x.v)) for m in mats for x in m)


def jcut_of(nsamp, fsamp, gauss):
    """bh_rf_axis_cut's first bin not formed (csrc/rf_plan.hip; N/2 + 1: all of them)"""
    half = nsamp // 2
    dw = 2.0 * np.pi * fsamp / nsamp
    jc = np.floor(RF_CUT_WA * gauss / dw) + 1.0
    return half + 1 if not (jc < half) else int(jc)


def spectrum(h, vp, vs, rho, p_s_per_deg, gauss, nsamp, fsamp, tshift, waveno, nsv=0.0, qp=None, qs=None):
    """One model (1-D float64 arrays of its nlay layers): X [N/2 + 1] clongdouble and its bounds E [2, N/2 + 1] (kernel set,
    IEEE set), or (None, None) for a model whose trace is NaN."""
    n = len(h)
    if n < 2:
        return None, None
    N, M = int(nsamp), int(nsamp) // 2
    qp = np.full(n, 500.0) if qp is None else np.asarray(qp, dtype=np.float64)
    qs = np.full(n, 225.0) if qs is None else np.asarray(qs, dtype=np.float64)
    p64 = float(p_s_per_deg) * 0.00899                  # (float64, as every implementation forms it)
    p = _t(LD(p64))
    z = np.zeros(n)                                      # float64 running sum, layer order
    acc = 0.0
    for i in range(n):
        z[i] = acc
        acc = acc + float(h[i])
    lay = []
    with np.errstate(all="ignore"):
        for i in range(n):
            zt = _t(LD(z[i]))
            hh = _T(LD(z[i + 1]) - LD(z[i]), U * abs(z[i + 1] - z[i])) if i < n - 1 else _t(LD(-1))
            lay.append(_flatten(zt, hh, _t(LD(vp[i])), _t(LD(vs[i])), _t(LD(rho[i]))))
        # t0: only its NaN-ness matters
        t0 = LD(0)
        for (d, a, b, _) in lay:
            v = a.v if waveno == 0 else b.v
            t0 += d.v * np.sqrt(1 / (v * v) - p.v * p.v)
        if not np.isfinite(t0):
            return None, None
        ru0, hm = _free_surface(p, lay[0][1], lay[0][2])
        ifc = [_interface(p, lay[i - 1][1], lay[i - 1][2], lay[i - 1][3], lay[i][1], lay[i][2], lay[i][3]) for i in range(1, n)]
        qfac = [(LD(1) / (PI * LD(qp[i])), LD(1) / (2 * LD(qp[i])), LD(1) / (PI * LD(qs[i])), LD(1) / (2 * LD(qs[i])))
                for i in range(n)]
        layvals = [x for (d, a, b, r) in lay for x in (d.v, 1 / (a.v * a.v), 1 / (b.v * b.v))] + [x for f in qfac for x in f]
        if not (np.all(np.isfinite(np.array(layvals, dtype=LD))) and _finite(ru0, hm, *[m for f in ifc for m in f])):
            return None, None
        # rotation (real)
        vs0, vp0 = LD(vs[0]), LD(vp[0])
        kap = vp0 / vs0
        poisson = (2 - kap * kap) / (2 - 2 * kap * kap)
        nsvv = LD(nsv) if nsv > 0 else vs0
        vptop, vstop = nsvv * np.sqrt((1 - poisson) / (LD(0.5) - poisson)), nsvv
        decomp = vstop > 0.01 and abs(p64) > 0.0001
        if decomp:
            P = p.v
            aa, bb = np.sqrt(1 / (vptop * vptop) - P * P), np.sqrt(1 / (vstop * vstop) - P * P)
            rot = [-(2 * vstop * vstop * P * P - 1) / (vptop * aa), 2 * P * vstop * vstop / vptop, -2 * P * vstop,
                   (1 - 2 * vstop * vstop * P * P) / (vstop * bb)]
            if not np.all(np.isfinite(np.array(rot, dtype=LD))):
                return None, None
            rot = [_T(r, 12 * U * abs(float(r))) for r in rot]

        # ---- every bin ----
        j = np.arange(M + 1)
        dw = 2 * PI * LD(fsamp) / LD(N)
        w = _T(dw * j.astype(LD), 3 * U * (dw * j).astype(np.float64))
        jj = np.maximum(j, 1).astype(LD)
        lg = np.where(j > 0, np.log(dw * jj / (2 * PI)), LD(0))
        lgw = _T(lg, 4 * U * np.abs(lg.astype(np.float64)) + 2 * U)
        p2 = p * p
        zero = _t(np.zeros(M + 1, dtype=CLD))
        q = g = nb = None
        for i in range(1, n):
            d, a, b, _ = lay[i - 1]
            ap, bp, as_, bs = qfac[i - 1]
            vcp = a * (lgw * ap + 1.0 + _t(CLD(1j) * bp))     # v (a + i b): the causal-Q velocity
            vcs = b * (lgw * as_ + 1.0 + _t(CLD(1j) * bs))
            sp = rcp(vcp * vcp) - p2
            ss = rcp(vcs * vcs) - p2
            plc, slc = csqrt(sp), csqrt(ss)
            wd = w * d
            mi = _t(CLD(-1j))
            e11 = cexp(mi * wd * plc)
            e22 = cexp(mi * wd * slc)
            if i == 1:
                nt = ru0
            else:
                rd_, td_, ru_, tu_ = ifc[i - 2]
                tq = _mat_mul(_mat_mul(td_, nb), q)
                nt = tuple(ru_[k] + tq[k] for k in range(4))
            e12 = e11 * e22
            nb = (nt[0] * (e11 * e11), nt[1] * e12, nt[2] * e12, nt[3] * (e22 * e22))
            rdn, tdn, run, tun = ifc[i - 1]
            rn = _mat_mul(rdn, nb)
            mm = (1.0 - rn[0], -rn[1], -rn[2], 1.0 - rn[3])
            idet = rcp(mm[0] * mm[3] - mm[1] * mm[2])
            minv = (idet * mm[3], -(idet * mm[1]), -(idet * mm[2]), idet * mm[0])
            q = _mat_mul(minv, tun)
            if i == 1:
                g = (e11 * q[0], e11 * q[1], e22 * q[2], e22 * q[3])
            else:
                g = _mat_mul((g[0] * e11, g[1] * e22, g[2] * e11, g[3] * e22), q)
        if waveno == 0:
            cr, cz = hm[0] * g[0] + hm[1] * g[2], hm[2] * g[0] + hm[3] * g[2]
        else:
            cr, cz = hm[0] * g[1] + hm[1] * g[3], hm[2] * g[1] + hm[3] * g[3]
        if decomp:
            cz, cr = cz * rot[0] + cr * rot[1], cz * rot[2] + cr * rot[3]
        if waveno == 1:
            cz, cr = cr, cz
        idn = rcp(cz * cz.conj())
        v = cr * cz.conj() * idn
        qg = _T(np.sqrt(PI) * LD(fsamp) / LD(gauss), 4 * U * float(np.sqrt(np.pi) * fsamp / gauss))
        wa = w * _t(LD(1) / LD(gauss))
        wa = _T(np.minimum(wa.v, LD(50)), np.where(wa.v > 50, 0.0, wa.e))
        ts = _t(LD(tshift))
        cq = qg * cexp(-0.25 * (wa * wa) + mi * (w * ts))
        X = v * cq
    E = X.e + 8 * U * _m(X.v)
    return X.v, E


class RfRef(object):
    """rf [B, nkeep] longdouble (NaN rows where the trace is NaN); bound, f64_bound, ref_bound: [B] float64, each good for every
    sample of the row; ill [B]: the bound is above the trace's peak (not asserted on); peak [B]."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def rf_ref(nlay, h, vp, vs, rho, p, gauss, nsamp, fsamp, tshift, waveno, nkeep, nsv=0.0, qp=None, qs=None,
           layout="layer_major"):
    """The reference of engine.rf_batch's call with the same arguments (host arrays, [Lmax, B] or [B, Lmax])."""
    arrs = [None if a is None else np.asarray(a, dtype=np.float64) for a in (h, vp, vs, rho, qp, qs)]
    if layout == "layer_major":
        arrs = [None if a is None else a.T for a in arrs]
    h, vp, vs, rho, qp, qs = arrs
    nlay = np.asarray(nlay)
    B, N, nkeep = len(nlay), int(nsamp), int(nkeep)
    M = N // 2
    wk = np.full(M + 1, 2.0)
    wk[0] = wk[M] = 1.0
    cut = np.arange(M + 1) >= jcut_of(N, fsamp, gauss)
    rf = np.full((B, nkeep), np.nan, dtype=LD)
    bound, f64b, refb, peak = (np.full(B, np.nan) for _ in range(4))
    eps_tw = np.array([4 * EPS_KERNEL["sin"] + 3 * U, 4 * EPS_F64["sin"] + 3 * U])
    for b in range(B):
        n = int(nlay[b])
        X, E = spectrum(h[b, :n], vp[b, :n], vs[b, :n], rho[b, :n], p, gauss, N, fsamp, tshift, waveno, nsv=nsv,
                        qp=None if qp is None else qp[b, :n], qs=None if qs is None else qs[b, :n])
        if X is None:
            continue
        with np.errstate(invalid="ignore"):
            f = np.fft.irfft(X, n=N)
        rf[b] = f[:nkeep]
        ax = _m(X)
        fft = (np.log2(N) + 4) * (4 * U + eps_tw) * np.sum(wk * ax) / N
        ek = np.sum(wk * (E[0] + np.where(cut, ax, 0.0))) / N + fft[0]
        ei = np.sum(wk * E[1]) / N + fft[1]
        refb[b] = (U_LD / U) * ei
        bound[b], f64b[b] = ek + refb[b], ei + refb[b]
        peak[b] = float(np.max(np.abs(f[:nkeep]))) if nkeep else 0.0
    with np.errstate(invalid="ignore"):
        ill = ~(bound <= np.maximum(peak, 0.0)) & np.isfinite(peak) & (peak > 0)
        ill |= ~np.isfinite(bound) & np.isfinite(peak)
    return RfRef(rf=rf, bound=bound, f64_bound=f64b, ref_bound=refb, ill=ill, peak=peak)


def check(got, ref, which="bound", factor=FACTOR, what=""):
    """|got - ref.rf| <= factor x ref.<which> on every row that is not ill; NaN rows of the reference must be NaN rows of `got`
    (and the other way round).  Returns (largest error / bound ratio over the checked rows, number of ill samples skipped)."""
    got = np.asarray(got, dtype=np.float64)
    want_nan = ~np.all(np.isfinite(ref.rf), axis=1)
    got_nan = ~np.all(np.isfinite(got), axis=1)
    assert np.array_equal(got_nan, want_nan), "%s: NaN rows %s, reference %s" % (what, np.flatnonzero(got_nan),
                                                                              np.flatnonzero(want_nan))
    bnd = getattr(ref, which)
    rows = np.flatnonzero(~want_nan & ~ref.ill)
    worst = 0.0
    for b in rows:
        diff = float(np.max(np.abs(got[b].astype(LD) - ref.rf[b]))) if got.shape[1] else 0.0
        ratio = diff / bnd[b] if bnd[b] > 0 else (0.0 if diff == 0 else np.inf)
        assert diff <= factor * bnd[b], ("%s: row %d: |diff| %.3e beyond %g x bound %.3e (peak %.3e)"
                                         % (what, b, diff, factor, bnd[b], ref.peak[b]))
        worst = max(worst, ratio)
    return worst, int(np.sum(ref.ill & ~want_nan)) * got.shape[1]
