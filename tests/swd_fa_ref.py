"""Extended-precision reference of the dispersion kernels' secular functions with an a priori error bound.

Not a conftest: a plain module the tests of the fast arithmetic import, like rf_ref.py.

What it computes
----------------
dltar1 (Love) and dltar4 (Rayleigh, no water layer) of surfdisp96.f:710-1068 -- with var (:874-991), dnka (:1024-1068) and normc
(:995-1020) -- for ONE model (binary32-valued d, a, b, rho of its mmax layers, the last one the half-space) at P points
(wvno, omega), in np.longdouble, from the formulas:

    per layer and wave type  xk = omega / v,  r^2 = (k + xk) |k - xk|,  r = sqrt(r^2),  q = r d
      k < xk (propagating)   cos q,  sin q / r,  -r sin q                                        scale 1
      k > xk (evanescent)    (1 + e^-2q) / 2,  (1 - e^-2q) / (2 r),  r (1 - e^-2q) / 2           scale e^-q  (var's exponent)
      Rayleigh               a0 = e^-(p + q) over the evanescent types, the ten products of var, the 19 entries of dnka,
                             e <- e CA, normc
      Love                   e1' = e1 cos + e2 mu z,  e2' = e1 y / mu + e2 cos,  the pair divided by its max-norm
    half-space               Rayleigh: the five entries of :800-808 from ra, rb;  Love: e1 = rho rb, e2 = 1 / beta^2

and returns the first entry of the surface vector divided by the vector's max-norm: e1 / max(|e1|, |e2|) for Love,
e[0] / max |e| for Rayleigh.  Every evaluator of the engine (the exact one, fa::*_secular, lean_*) returns this number up to
rounding whatever its normalisation cadence, because a positive scale factor of the vector cancels in it.  The reference's two
cut-offs (e^-2q taken as 0 from q = 16 on, a0 as 0 from p + q = 60 on) are NOT restated: the long-double value is the
function's; what they cost (e^-32 = 1.3e-14, e^-60) is charged to the bounds (below).

The bound
---------
A first-order running error analysis carried along with every value (class _T), as in rf_ref.py: every computed quantity x^
= x + dx carries E >= |dx|; u = 2^-53; contraction into FMAs only removes roundings.

    a + b   E_a + E_b + u |a + b|            a * b   |a| E_b + |b| E_a + u |a| |b|
    1 / v   (a model value or omega; exact input)   eps_rcp / |v|          (x / v is x * (1 / v): one more u)

Three epsilon sets are carried side by side:

    EPS_F64   correctly rounded operations and functions, u for each: the arithmetic of the reference (oracle.dltar)
    EPS_FA    the fast arithmetic of csrc/swd_fa.h (derived below)
    EPS_LD    this module's own arithmetic: the long double unit u_ld = 2^-64 for operations, 2 u_ld for library functions

    fa_bound = E[FA] + ref_bound,  f64_bound = E[F64] + ref_bound,  ref_bound = E[LD].

A positive factor common to a whole vector cancels in the result.  The analysis uses that three times: (1) the reciprocal of
a normalisation (IEEE division, or fa::rcp1 with its 2^-46) multiplies all entries alike, so an intermediate normc costs u per
entry and nothing else; only the LAST normalisation's reciprocal is charged, as eps_rcp1 |f|.  (2) Every entry of a layer's
matrix carries var's factor e^-(p + q) of its evanescent wave types; where the computed exponent differs from the true one, all
entries are off by the same factor.  (3) the final division by the max-norm |e_j|: df <= (E_0 + |f| E_j) / |e_j|.

A finite layer with k near xk.  cos(r d), sin(r d) / r and r sin(r d) are entire functions of t = -+ (r d)^2 (t < 0
propagating): C(t) = sum t^n / (2n)!, d S(t) with S(t) = sum t^n / (2n + 1)!, and (t / d) S(t), with C' = S / 2,
S' = (C - S) / (2 t), |S'| <= min(1/6, (1 + 1/q) / (2 q^2)) for t <= 0 and <= 0.2 for 0 < t < 1.  The error of t,
E_t = d^2 E_r2 + |t| (2 eps_sqrt + 3u), with E_r2 from the input error of k - xk (u (|k| + |xk|) plus the reciprocal's epsilon in
xk), goes through these derivatives -- not through sqrt and a division by r.  On the evanescent side with q < 1 the same is
done for the functions divided by the COMPUTED scale e^-q^ (form A; the scale is common to the layer, (2) above); with
q >= 1, where sqrt is harmless, the error dq = E_t / (2 q) goes through e^-2q directly (form B: no spurious u q from the
scale).  What stays near k = xk on the evanescent side is real: (1 - e^-2q) / 2 is formed by a subtraction in the reference's
arithmetic and in the fast one alike, so y = sinh-like / r is uncertain by eps_f / (2 r).  On the propagating side sin(q^) is
accurate relative to q for q < pi / 4 (the reduction leaves the argument alone), so nothing blows up there.

The half-space's ra, rb are true branch points: |sqrt(x + dx) - sqrt(x)| <= min(|dx| / (2 sqrt x), sqrt |dx|), plus
eps_sqrt sqrt(x).

Charged to BOTH arithmetic sets, so that f64_bound <= fa_bound holds by construction (the fast arithmetic has neither):
the reference's cut-offs (e^-2q for q >= 16 in the cos / sin-like terms, e^-(p+q) for p + q >= 60 in a0) and the rounding of
the sum p + q inside its a0 = exp(-(p + q)) (u (p + q) relative, up to 60 u).

EPS_FA, from the text of swd_fa.h
---------------------------------
seed   v_rcp_f64 / v_rsq_f64: relative error <= 2^-23.  ASSUMPTION: neither guide on the kernels' hardware states the accuracy
       of the binary64 seeds; this is the kernel's own "~2^-23" (swd_fa.h: sqrt_rsqrt).  Everything below needs only
       seed^4 << u, i.e. a seed better than ~2^-15.
rcp1   one Newton step r (1 + (1 - x r)): the error squares, the inner FMA's rounding is u * seed, the outer one's u:
       seed^2 + u <= 2^-46 + 2u (as rf_ref's rcp_nr).
rcp    a second step: (2^-46)^2 + u 2^-46 + u = u (1 + 2^-30) at most: 1 u.
sqrt_rsqrt  Goldschmidt on g -> sqrt x, h -> 1 / (2 sqrt x), relative errors a, b: one step maps them to (a - b) / 2 -
       (3/2) seed^2 (same for h with the sign of the first term reversed) plus the FMA's u.  a - b starts as the rounding of
       g = x y (u), so after step one |a - E|, |b - E| <= 1.5 u around a common E = 1.5 * 2^-46; step two leaves
       |a - b| / 2 <= 1.5 u, E^2 ~ 2^-90 and one more rounding: 2.5 u for s and for rs (= 2 h, exact).
sincos n = rint(x 2/pi) <= 57296 for x <= 9e4.  x - n pio2_1 is exact (pio2_1 has 33 bits, n 16: the product is exact and
       the difference a multiple of ulp(x) below x); the second FMA rounds once (u |r|); pio2_1 + pio2_1t misses pi / 2 by
       <= 2^-87, times n: 4e-22.  fdlibm's kernels are within 2^-58 on |r| <= pi / 4.  sin: r + r z ps -- the r^3 / 6 term
       (<= 0.103 |r|) with ~3 roundings, the last FMA's u |s|, the argument's u |r|: <= 2.4 u |r| + 4e-22.  cos: 1 - z / 2
       rounds at 1 (u), z's rounding enters as u z / 2 <= 0.31 u, the z^2 pc term 0.05 u, the argument's error |sin r| u |r|
       <= 0.56 u, the last FMA u: <= 2.95 u.  Either may come out as sin or cos: eps_sin = 3 u + 4e-22 ABSOLUTE on [0, 9e4],
       and for x < pi / 4 (n = 0) the sine is within sin_small |x| = 2.5 u |x|.
expneg n = rint(-x log2 e), |n| <= 1010; -x - n ln2_hi exact, second FMA u |r| <= 0.35 u, ln 2's two parts miss it by
       2^-86 n ~ 1e-23.  Taylor to r^12 on |r| <= ln 2 / 2: truncation r^13 / 13! = 1.7e-16, / e^r >= 0.707: 2.2 u.  Rounding of
       r + r^2 p (<= 0.41 + 0.27, relative to 0.707: 0.96 u) and of the final + 1 (u).  Total 4.5 u: eps_exp = 5 u RELATIVE on
       normal results (2^n is exact for x <= 700).
       In wave(): f = e^-2q is em * em: 2 eps_exp + u.  a0 = ep * eq: 2 eps_exp + u.
All four are below 8 u: the "within a few units in the last place" of swd_fa.h stands.  (rcp1's 2^-46 is not one of the four:
it only ever scales a whole vector.)

Tolerances are FACTOR x bound (FACTOR = 4, one constant), never fitted to what a GPU returns.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
U_LD = float(np.finfo(LD).eps) / 2.0
FACTOR = 4.0
POISON = 9.0e4                           # swd_fa.h wave() / love_terms(): arguments from here on poison the value (NaN)

EPS_FA = dict(rcp=U * (1 + 2.0 ** -30), rcp1=2.0 ** -46 + 2 * U, sqrt=2.5 * U + 2.0 ** -80, rsqrt=2.5 * U + 2.0 ** -80,
              sin=3 * U + 4e-22, sin_small=2.5 * U, exp=5 * U)
EPS_F64 = dict(rcp=U, rcp1=U, sqrt=U, rsqrt=U, sin=U, sin_small=U, exp=U)
EPS_LD = dict(rcp=U_LD, rcp1=U_LD, sqrt=2 * U_LD, rsqrt=2 * U_LD, sin=2 * U_LD, sin_small=2 * U_LD, exp=2 * U_LD)
_SETS = (EPS_FA, EPS_F64, EPS_LD)
UOP = np.array([U, U, U_LD]).reshape(3, 1)                     # one rounding of an operation, per set
_CUT = np.array([1.0, 1.0, 0.0]).reshape(3, 1)                 # the reference's cut-offs: charged to both arithmetic sets
_EPS_F = np.array([2 * EPS_FA["exp"] + U, U, 2 * U_LD]).reshape(3, 1)       # f = e^-2q: em * em, or one exp
_EPS_A0 = np.array([2 * EPS_FA["exp"] + U, U, 2 * U_LD]).reshape(3, 1)      # a0: ep * eq, or one exp (plus u (p + q), below)


def _eps(name):
    return np.array([s[name] for s in _SETS]).reshape(3, 1)


def _m(x):
    with np.errstate(over="ignore"):
        return np.abs(x).astype(np.float64)


class _T(object):
    """A value (long double [P]) and its error bounds [3, P] (FA, F64, LD)."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = v
        e = np.asarray(e, dtype=np.float64)
        self.e = e if e.ndim == 2 else np.broadcast_to(e, (3,) + (np.shape(v) or (1,)))

    def __add__(self, o):
        o = _t(o)
        v = self.v + o.v
        return _T(v, self.e + o.e + UOP * _m(v))

    __radd__ = __add__

    def __sub__(self, o):
        o = _t(o)
        v = self.v - o.v
        return _T(v, self.e + o.e + UOP * _m(v))

    def __rsub__(self, o):
        return _t(o) - self

    def __neg__(self):
        return _T(-self.v, self.e)

    def __mul__(self, o):
        if isinstance(o, (int, float)) and abs(o) in (1.0, 2.0, 0.5):          # exact
            return _T(self.v * LD(o), self.e * abs(o))
        o = _t(o)
        a, b = _m(self.v), _m(o.v)
        return _T(self.v * o.v, a * o.e + b * self.e + UOP * a * b)

    __rmul__ = __mul__


def _t(x):
    return x if isinstance(x, _T) else _T(np.asarray(x, dtype=LD))


def _inv(v):
    """1 / v of an exact input (a model value or omega): IEEE division, fa::rcp"""
    w = 1 / np.asarray(v, dtype=LD)
    return _T(w, _eps("rcp") * _m(w))


def _sqrt_branch(x):
    """sqrt at a true branch point (the half-space's ra, rb)"""
    v = np.sqrt(x.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        lin = x.e / (2 * _m(v))
    lin = np.where(np.isfinite(lin), lin, np.inf)
    return _T(v, np.minimum(lin, np.sqrt(x.e)) + _eps("sqrt") * _m(v))


def _r2(k, xk):
    """r^2 = (k + xk) |k - xk| with the input error of k - xk; also k - xk"""
    dk = k - xk
    sp = k + xk
    return _T(sp.v * np.abs(dk.v), _m(dk.v) * sp.e + _m(sp.v) * dk.e + UOP * _m(sp.v * dk.v)), dk.v


class _Wave(object):
    __slots__ = ("cs", "y", "z", "ex", "dqb", "q", "qe")


def _wave(k, xk, d):
    """One wave type of one finite layer: cs, y (sin-like / r), z (-+ r sin-like) in var's scaling, the exponent ex, the error dqb
    of the exponent where it is carried explicitly (form B), and q = r d with its bound."""
    r2, dk = _r2(k, xk)
    dm = float(d)
    rb = np.sqrt(r2.v)
    q = rb * d
    qf, rbf, r2f = _m(q), _m(rb), _m(r2.v)
    tabs = qf * qf
    et = dm * dm * r2.e + tabs * (2 * _eps("sqrt") + 3 * UOP)
    evan = dk > 0
    w = _Wave()
    with np.errstate(all="ignore"):
        small = qf < np.pi / 4
        # ---- propagating
        C, Sn = np.cos(q), np.sin(q)
        S = np.where(qf > 0, _m(Sn) / np.where(qf > 0, qf, 1.0), 1.0)
        esin = np.where(small, _eps("sin_small") * qf, _eps("sin"))
        dS = np.minimum(1.0 / 6.0, np.where(qf > 0, (1 + 1 / qf) / (2 * tabs), np.inf))
        yp = np.where(qf > 0, Sn / np.where(qf > 0, rb, 1), LD(d))
        zp = -(rb * Sn)
        e_cp = S / 2 * et + _eps("sin")
        e_yp = dm * dS * et + np.where(small, dm * _eps("sin_small"), esin / rbf) + _m(yp) * (_eps("rsqrt") + _eps("sqrt") + 2 * UOP)
        e_zp = (S + np.abs(_m(C) - S) / 2) * et / dm + rbf * esin + _m(zp) * (_eps("sqrt") + 2 * UOP)
        # ---- evanescent, var's scaling e^-q
        f = np.exp(-2 * q)
        cs = (1 + f) / 2
        sn = -np.expm1(-2 * q) / 2
        ff, csf, snf = _m(f), _m(cs), _m(sn)
        dfr = _EPS_F * ff + _CUT * np.where(qf >= 16.0, ff, 0.0)
        ye = sn / rb
        ze = rb * sn
        A = qf < 1.0
        Ss = np.where(qf > 0, snf / np.where(qf > 0, qf, 1.0), 1.0)
        dsn = dfr / 2 + UOP * snf
        # form A
        a_cs = Ss / 2 * et + dfr / 2 + UOP * csf
        a_y = dm * 0.2 * et + dsn / rbf + _m(ye) * (_eps("sqrt") + _eps("rsqrt") + 2 * UOP)
        a_z = (Ss + np.abs(csf - Ss) / 2) * et / dm + rbf * dsn + _m(ze) * (_eps("sqrt") + 2 * UOP)
        # form B
        dq = et / (2 * qf)
        df = 2 * ff * dq + dfr
        b_cs = df / 2 + UOP * csf
        b_sn = df / 2 + UOP * snf
        relr = r2.e / (2 * r2f)
        b_y = b_sn / rbf + _m(ye) * (relr + _eps("rsqrt") + 2 * UOP)
        b_z = rbf * b_sn + _m(ze) * (relr + _eps("sqrt") + 2 * UOP)
        e_ce = np.where(A, a_cs, b_cs)
        e_ye = np.where(A, a_y, b_y)
        e_ze = np.where(A, a_z, b_z)
        w.cs = _T(np.where(evan, cs, C), np.where(evan, e_ce, e_cp))
        w.y = _T(np.where(evan, ye, yp), np.where(evan, e_ye, e_yp))
        w.z = _T(np.where(evan, ze, zp), np.where(evan, e_ze, e_zp))
        w.ex = np.where(evan, q, LD(0))
        w.dqb = np.where(evan & ~A, dq, 0.0)
        w.q = q
        qe = np.where(rbf > 0, dm * r2.e / (2 * rbf), np.sqrt(r2.e) * dm) + qf * (_eps("sqrt") + UOP)
        w.qe = qe[0] + qe[2]
    return w


def _normalize(vec):
    """normc: the vector by its max-norm; returns the index of the largest entry as well"""
    mags = np.stack([np.abs(x.v) for x in vec])
    j = np.argmax(mags, axis=0)
    m = np.max(mags, axis=0)
    m = np.where(m < LD(1e-40), LD(1), m)
    mf = _m(m)
    out = []
    for x in vec:
        v = x.v / m
        out.append(_T(v, x.e / mf + UOP * _m(v)))
    return out, j


class SecRef(object):
    """value [P] longdouble; fa_bound, f64_bound, ref_bound [P] float64; q [nq, P] longdouble: r d of every finite layer's wave
    types (Rayleigh: P then S per layer) with q_bound [nq, P], the fast arithmetic's error of it (for the poison rule)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def secular_ref(ifunc, d, a, b, rho, wvno, omega):
    """ifunc 1 Love, 2 Rayleigh.  d, a, b, rho: the model's mmax layers (binary32 values).  wvno, omega: [P] float64."""
    d, a, b, rho = [np.asarray(np.asarray(x, dtype=np.float32), dtype=LD) for x in (d, a, b, rho)]
    mmax = d.size
    assert mmax >= 2 and ifunc in (1, 2)
    k = _t(np.asarray(wvno, dtype=np.float64).astype(LD))
    om = _t(np.asarray(omega, dtype=np.float64).astype(LD))
    P = k.v.shape
    qs, qes = [], []
    with np.errstate(all="ignore"):
        if ifunc == 1:
            ib = _inv(b[-1])
            r2, _ = _r2(k, om * ib)
            vec = [_t(np.full(P, rho[-1])) * _sqrt_branch(r2), _t(np.full(P, 1.0, dtype=LD)) * (ib * ib)]
            for m in range(mmax - 2, -1, -1):
                ib = _inv(b[m])
                wv = _wave(k, om * ib, d[m])
                qs.append(wv.q)
                qes.append(wv.qe)
                yx = wv.y * (ib * ib * _inv(rho[m]))
                zx = wv.z * (_t(rho[m]) * _t(b[m]) * _t(b[m]))
                e1, e2 = vec
                vec, j = _normalize([e1 * wv.cs + e2 * zx, e1 * yx + e2 * wv.cs])
        else:
            iom = _inv(om.v)
            k2 = k * k
            t = _t(b[-1]) * iom
            gammk = 2.0 * (t * t)
            gam = gammk * k2
            gamm1 = gam - 1.0
            r2a, _ = _r2(k, om * _inv(a[-1]))
            r2b, _ = _r2(k, om * _inv(b[-1]))
            ra, rb = _sqrt_branch(r2a), _sqrt_branch(r2b)
            rarb = ra * rb
            r1 = _t(rho[-1])
            vec = [r1 * r1 * (gamm1 * gamm1 - gam * gammk * rarb), -(r1 * ra), r1 * (gamm1 - gammk * rarb), r1 * rb, k2 - rarb]
            for m in range(mmax - 2, -1, -1):
                t = _t(b[m]) * iom
                gammk = 2.0 * (t * t)
                gam = gammk * k2
                wp = _wave(k, om * _inv(a[m]), d[m])
                ws = _wave(k, om * _inv(b[m]), d[m])
                qs += [wp.q, ws.q]
                qes += [wp.qe, ws.qe]
                exa = wp.ex + ws.ex
                a0v = np.exp(-exa)
                a0f, exf = _m(a0v), _m(exa)
                a0 = _T(a0v, a0f * (_EPS_A0 + _CUT * U * exf + UOP * exf * (1 - _CUT) + wp.dqb + ws.dqb)
                        + _CUT * (np.where(exf >= 60.0, a0f, 0.0) + np.where((_m(wp.ex) > 700) | (_m(ws.ex) > 700), 1e-300, 0.0)))
                cosp, w, x, cosq, y, z = wp.cs, wp.y, wp.z, ws.cs, ws.y, ws.z
                cpcq, cpy, cpz, cqw, cqx = cosp * cosq, cosp * y, cosp * z, cosq * w, cosq * x
                xy, xz, wy, wz = x * y, x * z, w * y, w * z
                rh, irh = _t(rho[m]), _inv(rho[m])
                gamm1 = gam - 1.0
                twgm1 = gam + gamm1
                gmgmk, gmgm1, gm1sq = gam * gammk, gam * gamm1, gamm1 * gamm1
                rho2, irho2 = rh * rh, irh * irh
                a0pq = a0 - cpcq
                ca11 = cpcq - 2.0 * (gmgm1 * a0pq) - gmgmk * xz - k2 * gm1sq * wy
                ca12 = (k2 * cpy - cqx) * irh
                ca13 = -((twgm1 * a0pq + gammk * xz + k2 * gamm1 * wy) * irh)
                ca14 = (cpz - k2 * cqw) * irh
                ca15 = -((2.0 * (k2 * a0pq) + xz + k2 * k2 * wy) * irho2)
                ca21 = (gmgmk * cpz - gm1sq * cqw) * rh
                ca22 = cpcq
                ca23 = gammk * cpz - gamm1 * cqw
                ca24 = -wz
                ca41 = (gm1sq * cpy - gmgmk * cqx) * rh
                ca42 = -xy
                ca43 = gamm1 * cpy - gammk * cqx
                ca51 = -((2.0 * (gmgmk * gm1sq * a0pq) + gmgmk * gmgmk * xz + gm1sq * gm1sq * wy) * rho2)
                ca53 = -((gammk * gamm1 * twgm1 * a0pq + gam * gammk * gammk * xz + gamm1 * gm1sq * wy) * rh)
                tt = -2.0 * k2
                ca31, ca32, ca34, ca35 = tt * ca53, tt * ca43, tt * ca23, tt * ca13
                ca33 = a0 + 2.0 * (cpcq - ca11)
                ca25, ca44, ca45, ca52, ca54, ca55 = ca14, ca22, ca12, ca41, ca21, ca11
                ca = [[ca11, ca12, ca13, ca14, ca15], [ca21, ca22, ca23, ca24, ca25], [ca31, ca32, ca33, ca34, ca35],
                      [ca41, ca42, ca43, ca44, ca45], [ca51, ca52, ca53, ca54, ca55]]
                e = vec
                ee = []
                for i in range(5):
                    s = e[0] * ca[0][i]
                    for jj in range(1, 5):
                        s = s + e[jj] * ca[jj][i]
                    ee.append(s)
                vec, j = _normalize(ee)
        f = vec[0]
        ej = np.stack([x.e for x in vec])                       # [n, 3, P]
        ejm = np.take_along_axis(ej, j[None, None, :].repeat(3, axis=1), axis=0)[0]
        E = f.e + _m(f.v) * (ejm + _eps("rcp1"))
    E = np.where(np.isfinite(E), E, np.inf)
    return SecRef(value=f.v, fa_bound=E[0] + E[2], f64_bound=E[1] + E[2], ref_bound=E[2],
                  q=np.stack(qs), q_bound=np.stack(qes))


# ---- the population of the tests (fixed seeds) --------------------------------------------------------------------------------
LAYER_COUNTS = (2, 3, 4, 5, 12, 32)


def sorted_model(rs, mmax):
    """velocities increasing with depth"""
    vs = np.sort(rs.uniform(1.5, 4.8, mmax)).astype(np.float32)
    vp = (vs * rs.uniform(1.65, 1.9, mmax)).astype(np.float32)
    vp = np.sort(vp)
    rho = (0.77 + 0.32 * vp).astype(np.float32)
    d = rs.uniform(0.5, 8.0, mmax).astype(np.float32)
    d[-1] = 0.0
    return d, vp, vs, rho


def lvz_model(rs, mmax):
    """the same with one low-velocity layer (where the model has an inner layer to lower)"""
    d, vp, vs, rho = sorted_model(rs, mmax)
    if mmax >= 3:
        i = int(rs.randint(1, mmax - 1))
        vs[i] = np.float32(0.7 * vs[i - 1])
        vp[i] = np.float32(0.75 * vp[i - 1])
    return d, vp, vs, rho


def corner_model():
    """the corners of SearchT::init's sanity bounds"""
    d = np.array([1e-3, 9.9e6, 3.0, 0.0], dtype=np.float32)
    vp = np.array([100.0, 100.0, 5.0, 100.0], dtype=np.float32)
    vs = np.array([57.0, 57.0, 2.8, 57.0], dtype=np.float32)
    rho = np.array([999999.0, 0.001, 2.5, 999999.0], dtype=np.float32)
    return d, vp, vs, rho


def points(rs, ifunc, d, vp, vs, n=64):
    """(period, c) points of one model: n / 2 uniform over 0.8 vs_min .. vs_max, n / 4 within 10^-U(6, 12) relative of a layer's
    vs (or vp, Rayleigh) on either side, the rest at the same distances from the half-space's.  Returns wvno, omega, kind
    (0 uniform, 1 near a layer velocity, 2 near a half-space velocity) and the relative distance (0 for uniform points)."""
    per = rs.uniform(0.5, 100.0, n)
    omega = 2 * np.pi / per
    c = rs.uniform(0.8 * vs.min(), vs.max(), n)
    kind = np.zeros(n, dtype=int)
    dist = np.zeros(n)
    for i in range(n // 2, n):
        hs = i >= n // 2 + n // 4
        m = len(vs) - 1 if hs else int(rs.randint(0, len(vs)))
        v = float(vp[m] if (ifunc == 2 and rs.rand() < 0.5) else vs[m])
        dist[i] = 10.0 ** -rs.uniform(6, 12)
        c[i] = v * (1 + dist[i] * (1 if rs.rand() < 0.5 else -1))
        kind[i] = 2 if hs else 1
    return omega / c, omega, kind, dist


def population(seed=20):
    """[(name, ifunc, (d, vp, vs, rho), wvno, omega, kind, dist)]: per wave type and layer count a sorted and an LVZ model, and the
    bound-corner model"""
    rs = np.random.RandomState(seed)
    out = []
    for ifunc in (1, 2):
        for mmax in LAYER_COUNTS:
            for name, gen in (("sorted", sorted_model), ("lvz", lvz_model)):
                d, vp, vs, rho = gen(rs, mmax)
                out.append(("%s%d" % (name, mmax), ifunc, (d, vp, vs, rho)) + points(rs, ifunc, d, vp, vs))
        d, vp, vs, rho = corner_model()
        out.append(("corner", ifunc, (d, vp, vs, rho)) + points(rs, ifunc, d, vp, vs))
    return out
