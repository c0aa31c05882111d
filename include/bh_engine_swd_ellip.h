/*
 * include/bh_engine_swd_ellip.h -- Rayleigh-wave ellipticity (H/V, the ZH ratio) of the fundamental mode: libbh_engine.so.
 *
 * An extension outside the drop-in contract of include/bh_engine.h (the reference has no such target).  The dispersion search
 * propagates Dunkin's five-component compound vector e from the half-space to the surface and keeps e[0], whose zero is the phase
 * velocity.  At that zero the ratio of two other components is the ellipticity: this call evaluates the same function a few more
 * times per (model, period) and returns it.  bayhunter_amd/csrc/swd_ellip.hip; tests/ellip_ref.py restates everything below in
 * plain Python, and the kernel returns its bits.
 *
 * THE FUNCTION.  All in float64, no product and sum contracted, sqrt and division correctly rounded, sincos and exp those of
 * glibc (bh_libm.h).  The model is read as the dispersion kernels read it: h, vp, vs, rho of layer l are (double)(float) of the
 * array's value, d, a, b, r below; layer mmax-1 (mmax = nlay[b]) is the half-space.  For period T and phase velocity c:
 *     omega = (2.0 * 3.141592653589793) / T,   k = wvno = omega / c,   om = omega < 1e-4 ? 1e-4 : omega,   k2 = k * k
 *   per layer (half-space included):  xka = om / a,  xkb = om / b,  ra = sqrt((k + xka) * fabs(k - xka)),
 *     rb = sqrt((k + xkb) * fabs(k - xkb)),  t = b / om,  gammk = 2.0 * t * t,  gam = gammk * k2,  gamm1 = gam - 1.0
 *   start (half-space):  e[0] = r * r * (gamm1 * gamm1 - gam * gammk * ra * rb),  e[1] = -r * ra,
 *     e[2] = r * (gamm1 - gammk * ra * rb),  e[3] = r * rb,  e[4] = k2 - ra * rb
 *   then for m = mmax-2 down to 0:  p = ra * d,  q = rb * d, the layer's eigenfunction products and compound matrix
 *     (surfdisp96.f:874-991 `var`, :1024-1068 `dnka`, in the reference's operation order), e <- e * CA accumulated from 0.0 in
 *     index order, then `normc`: e <- e / max|e[i]| (the maximum replaced by 1.0 where it is below 1e-40).
 *   E(c) = that vector after the last layer; e0(c) = E(c)[0], the reference's secular function up to the positive norm.
 *
 * THE RATIOS, from E = E(c) and k = omega / c:
 *     hv     =  E[3] / (k * E[2])
 *     hv_alt = -k * E[2] / E[1]
 *     mismatch = fabs(hv - hv_alt) / fabs(hv)
 * Both are the surface u_r / u_z of the fundamental mode AT a root of e0; POSITIVE MEANS RETROGRADE particle motion (a
 * homogeneous half-space: hv = 2 sqrt(1 - c^2/b^2) / (2 - c^2/b^2) > 0), negative prograde.  Off the root the two move in opposite
 * directions, so mismatch bounds the error of hv that a c which is not quite the root leaves (measured: error <= 0.87 x
 * mismatch on four well-behaved stacks).  |d ln hv / d ln c| is 8 to 30 on those stacks at 4 to 40 s, more at an H/V peak; on models
 * of the kind a chain proposes (velocities in any order; tests/golden/ellip_exact.npz, against a 110-digit reference) it is 1.1 to
 * 2.4e3 where two polish steps converge and 1.4e5 to 2.2e9 where they do not: a mode trapped in a low-velocity channel has
 * almost no surface expression, e0 goes from -1 to 1 between neighbouring doubles, and a c good to the last bit leaves hv
 * undetermined.  mismatch is O(1) there.  (The two expressions also meet where the displacement minor vanishes instead of the
 * traction minor, so a small mismatch is a necessary sign of a root, not a proof of one.)
 *
 * THE GATE.  An entry whose mismatch is not <= BH_ELLIP_MISMATCH_MAX raises the flag, exactly like a polish step that leaves the
 * window: an ellipticity that the arithmetic does not determine is not a value.  hv, mismatch and cpol are written as computed.
 * The constant: the largest mismatch of an entry the tests take as a value -- unpolished, from a velocity within the search's 2e-6
 * of the root -- is 2.5e-4 (profiles/swd_ellip_accuracy.txt); the smallest power of ten at least ten times that.  For an entry
 * that passes, |atan(hv) - atan(hv at the root)| <= BH_ELLIP_MISMATCH_MAX where the root's value lies between the two expressions.
 *
 * THE POLISH, nsteps = 0..3 secant steps on e0 from the c handed in (the search's c is within ~2e-6 of the root):
 *     nsteps == 0:  E = E(c), cpol = c.
 *     else:  c0 = c;  c1 = c0 * (1.0 + 0x1p-20);  f0 = e0(c0);  f1 = e0(c1)
 *            repeat nsteps times:
 *                if f1 == f0: stop
 *                c2 = c1 - f1 * (c1 - c0) / (f1 - f0)
 *                if not fabs(c2 - c) <= 1e-5 * c:   (the step left the window, or is not a number)
 *                    E = E(c), cpol = c, the flag is set, stop
 *                c0 = c1;  f0 = f1;  c1 = c2;  f1 = e0(c1)
 *            E = the last evaluation made, cpol = the velocity it was made at.
 * The window 1e-5 c is the agreement this library promises with the reference's velocities: a step that leaves it has found
 * another root, and the lane falls back to the unpolished value.  Two steps leave hv within 1e-12 of its value at the root
 * whichever search produced c (tests/test_ellip_ref.py).
 *
 * PER (model, period):
 *   - no root -- err[b] != 0, or vel <= 0 (or not a number), or nlay[b] outside 1..Lmax: hv = mismatch = cpol = 0, nothing is
 *     evaluated, no flag.  The zero rows of a failed dispersion search stay zero rows.
 *   - (float)vs of the top layer <= 0 (a water layer; not supported), E[1] == 0, E[2] == 0, or one of hv, hv_alt, mismatch not
 *     finite: hv = mismatch = NaN, cpol as above, the flag is set.
 *   - mismatch > BH_ELLIP_MISMATCH_MAX (the gate): the flag is set, the values stay.
 * flag[b] = 1 if any of model b's K entries set the flag, else 0.
 *
 * Errors leave their message in bh_engine_last_error.  BH_EINVAL launches nothing and writes nothing.
 */
#ifndef BH_ENGINE_SWD_ELLIP_H
#define BH_ENGINE_SWD_ELLIP_H

#include "bh_engine.h"

#define BH_ELLIP_MISMATCH_MAX 1.0e-2 /* the gate above */

#ifdef __cplusplus
extern "C" {
#endif

/* B models (nlay, h, vp, vs, rho, stride_l, stride_b, memspace, stream: as bh_swd_batch), K = 1..60 periods [s], nsteps = 0..3.
 *   have_vel == 0: the engine first runs its own fundamental-mode Rayleigh phase-velocity search (iwave 2, igr 0, mode 1, flsph 0,
 *                  with the search and arithmetic it is set to) into vel / err, then the ellipticity kernel on the same stream.
 *   have_vel != 0: vel [B*K] and err [B] are read.
 *   hv [B*K] float64; mismatch [B*K], cpol [B*K] float64, may be NULL; flag [B] int32.
 * BH_EINVAL: B < 0, Lmax outside 1..100, strides <= 0, K outside 1..60, nsteps outside 0..3, a null nlay, h, vp, vs, rho, periods,
 * vel, err, hv or flag.  memspace BH_DEVICE only enqueues; BH_HOST returns with the results on the host. */
int bh_swd_ellip(bh_engine *e, int memspace, void *stream, int B, int Lmax, const int32_t *nlay, const double *h, const double *vp,
                 const double *vs, const double *rho, ptrdiff_t stride_l, ptrdiff_t stride_b, int K, const double *periods,
                 int have_vel, double *vel, int32_t *err, int nsteps, double *hv, double *mismatch, double *cpol, int32_t *flag);

#ifdef __cplusplus
}
#endif
#endif
