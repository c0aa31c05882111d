"""The Rayleigh ellipticity of the fundamental mode to 100+ digits, sharing no formula with the library: mpmath only, no GPU, nothing of
the project imported.

The motion-stress vector r = (r1, r2, r3, r4) of Aki & Richards (7.28), dr/dz = A r with u_x = r1 e^{i(kx - wt)},
u_z = i r2 e^{i(kx - wt)}, z downward.  The two solutions that decay in the half-space are carried up to the free surface through
expm(-A h) of every layer, each column rescaled after every layer (the minors below are ratios, or a sign).  With Y the [4, 2]
result and m(i, j) = Y[i, 0] Y[j, 1] - Y[i, 1] Y[j, 0]:
    the secular function is the traction minor m(2, 3): zero where a combination of the two has no traction at the surface;
    at such a root the surface u_x / u_z of that combination is m(0, 2) / m(1, 2) = m(0, 3) / m(1, 3);
    hv = -m(0, 2) / m(1, 2): the library's sign, positive = retrograde.
The model is what the kernels read -- every layer value rounded to binary32, taken as the exact rational it then is -- and
omega = 2.0 * 3.141592653589793 / T as float64 arithmetic forms it, taken exactly likewise.

Precision.  Both columns grow upwards like exp(nu_b h), their minors like exp((nu_a + nu_b) h): the minors lose
exp((nu_b - nu_a) h) <= exp(k h) to cancellation per layer.  The working precision is DIGITS plus the decimal digits of
exp(k sum(h)), so what is left is DIGITS whatever the stack and the period.

A mode trapped in a deep low-velocity channel reaches the surface with an amplitude of 1e-40 or less of its size in the channel, and
all six minors are then that small at the root: the two expressions of hv agree only once c* is known to many more digits than
that.  `ellipticity` therefore repeats the secant at twice the digits and a squared tolerance (LADDER) until they agree."""
import mpmath as mp

DIGITS = 110
LADDER = ((110, -80), (220, -180), (440, -380))   # (digits, log10 of the secant's last relative step)
TWOPI = 2.0 * 3.141592653589793


def exact_model(h, vp, vs, rho):
    """one model's own layers (the last is the half-space), checked to be binary32 values -> four lists of Python floats"""
    import struct
    out = []
    for arr in (h, vp, vs, rho):
        col = []
        for v in arr:
            v = float(v)
            assert struct.unpack("f", struct.pack("f", v))[0] == v, "a layer value that is no binary32 value"
            col.append(v)
        out.append(col)
    return out


def _matrix(k, w, alpha, beta, rho):
    mu = rho * beta * beta
    l2m = rho * alpha * alpha
    lam = l2m - 2 * mu
    zeta = 4 * mu * (lam + mu) / l2m
    return mp.matrix([[0, k, 1 / mu, 0],
                      [-k * lam / l2m, 0, 0, 1 / l2m],
                      [k * k * zeta - w * w * rho, 0, 0, k * lam / l2m],
                      [0, -w * w * rho, -k, 0]])


class Surface(object):
    """the two solutions at the free surface of `model` at period T and phase velocity c (an mpf or a float, taken exactly)"""

    def __init__(self, model, T, c, digits=DIGITS):
        h, vp, vs, rho = model
        n = len(vs)
        if not float(c) < vs[n - 1]:
            raise ValueError("c at or above the half-space's S velocity: no decaying S solution")
        if not min(vs) > 0.0:
            raise ValueError("a fluid layer")
        depth = sum(h[:n - 1])
        with mp.workdps(30):
            grow = float(mp.mpf(TWOPI / float(T)) / mp.mpf(c) * depth / mp.log(10))
        self.dps = digits + int(grow) + 10
        with mp.workdps(self.dps):
            w = mp.mpf(TWOPI / float(T))
            k = w / mp.mpf(c)
            a, b, r = mp.mpf(vp[n - 1]), mp.mpf(vs[n - 1]), mp.mpf(rho[n - 1])
            mu, l2m = r * b * b, r * a * a
            lam = l2m - 2 * mu
            Y = mp.matrix(4, 2)
            for j, v in enumerate((a, b)):   # potentials exp(-nu z): (r1, r2) = (k, nu_a) for P, (nu_b, k) for SV
                nu = mp.sqrt(k * k - (w / v) ** 2)
                r1, r2 = (k, nu) if j == 0 else (nu, k)
                col = [r1, r2, mu * (-nu * r1 - k * r2), -l2m * nu * r2 + k * lam * r1]
                for i in range(4):
                    Y[i, j] = col[i]
                res = _matrix(k, w, a, b, r) * Y[:, j] + nu * Y[:, j]   # an eigenvector of eigenvalue -nu
                assert max(abs(x) for x in res) <= mp.mpf(10) ** -(digits - 10) * max(abs(x) for x in col) * (k + w) ** 2
            for m in range(n - 2, -1, -1):   # r(top) = expm(-A h) r(bottom)
                Y = mp.expm(-_matrix(k, w, mp.mpf(vp[m]), mp.mpf(vs[m]), mp.mpf(rho[m])) * mp.mpf(h[m])) * Y
                for j in range(2):
                    s = max(abs(Y[i, j]) for i in range(4))
                    for i in range(4):
                        Y[i, j] = Y[i, j] / s
            self.Y = Y

    def minor(self, i, j):
        Y = self.Y
        with mp.workdps(self.dps):   # (the cancellation the extra digits are there for happens here)
            return Y[i, 0] * Y[j, 1] - Y[i, 1] * Y[j, 0]


def secular(model, T, c, digits=DIGITS):
    """the traction minor m(2, 3)"""
    return Surface(model, T, c, digits).minor(2, 3)


def root(model, T, c, tol=1e-80, window=1e-5, maxit=80, digits=DIGITS):
    """The root of `secular` next to c by the secant from c and c (1 + 1e-9), to a relative step of tol; None where an iterate
    leaves c (1 +- window), reaches the half-space's S velocity, or the steps do not shrink below tol in maxit."""
    with mp.workdps(digits):
        c = mp.mpf(c)
        top = mp.mpf(model[2][-1])
        tol, window = mp.mpf(tol), mp.mpf(window)
        if not c < top:
            return None
        c0, c1 = c, c * (1 + mp.mpf(10) ** -9)
        if not c1 < top:
            c1 = c * (1 - mp.mpf(10) ** -9)
        f0, f1 = secular(model, T, c0, digits), secular(model, T, c1, digits)
        for _ in range(maxit):
            if f1 == f0:
                return None
            c2 = c1 - f1 * (c1 - c0) / (f1 - f0)
            if not abs(c2 - c) <= window * c or not c2 < top:
                return None
            c0, f0 = c1, f1
            c1, f1 = c2, secular(model, T, c2, digits)
            if abs(c1 - c0) <= tol * abs(c1):
                return c1
        return None


def hv_at(model, T, cstar, digits=DIGITS):
    """(hv, hv') = (-m(0,2)/m(1,2), -m(0,3)/m(1,3)) at cstar; at a root the two agree"""
    s = Surface(model, T, cstar, digits)
    with mp.workdps(s.dps):
        return -s.minor(0, 2) / s.minor(1, 2), -s.minor(0, 3) / s.minor(1, 3)


def ellipticity(model, T, c):
    """(c*, hv*, the digits of LADDER it took) of the root next to c, or None (see `root`).  The two expressions of hv* must
    agree to 1e-15."""
    for digits, tol in LADDER:
        with mp.workdps(digits):
            cstar = root(model, T, c, tol=mp.mpf(10) ** tol, digits=digits)
            if cstar is None:
                return None
            a, b = hv_at(model, T, cstar, digits)
            if abs(a - b) <= mp.mpf(10) ** -20 * abs(a):
                break
    with mp.workdps(DIGITS):
        assert abs(a - b) <= mp.mpf(10) ** -15 * abs(a), "the two expressions of hv disagree at the root: %s %s" % (a, b)
        return +cstar, +a, digits
