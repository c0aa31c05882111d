// bayhunter_amd/csrc/swd_ellip.hip -- Rayleigh-wave ellipticity (H/V) of the fundamental mode (include/bh_engine_swd_ellip.h).
//
// The dispersion kernels propagate Dunkin's compound vector e from the half-space to the surface and keep e[0]; at its zero
// e[3] / (k e[2]) = -k e[2] / e[1] is the surface u_r / u_z.  One lane = one (model, period), lane b*K + k: the lanes of a model are
// neighbours and read the same layer values from global memory (one cache line per layer and array, broadcast), a wavefront
// loops to the largest layer count among its lanes with the shallower ones predicated off.  A lane makes at most nsteps + 2
// evaluations of the compound vector -- the secant polish of the header -- against the ~50 rounds of the search before it.
//
// The arithmetic is the reference's, operation for operation: layer_products, rayleigh_ca19 and rayleigh_apply<true> of
// swd_common.h (the code of rayleigh_secular<true>), glibc's sincos / exp through bh_libm.h, -ffp-contract=off.
#include "../../include/bh_engine_swd_ellip.h"
#include "bh_device.h"
#include "bh_hostkit.h"
#include <cmath>

#define BH_HD __device__ __forceinline__
#define BH_TAB static __device__ const
#include "bh_libm.h"

namespace {
#include "swd_common.h"

constexpr int ELLIP_THREADS = 256; // four wavefronts share one copy of the libm tables
constexpr int ELLIP_LDS = (LIBM_TAB_BYTES + 15) & ~15;

// a model's layers where the caller left them, rounded to binary32 as the dispersion kernels stage them (swd_kernel.hip)
struct ModelGlobal {
    const double *h, *vp, *vs, *rho; // pre-offset to the model
    ptrdiff_t sl;
    __device__ __forceinline__ double D(int m) const { return (double)(float)h[(ptrdiff_t)m * sl]; }
    __device__ __forceinline__ double A(int m) const { return (double)(float)vp[(ptrdiff_t)m * sl]; }
    __device__ __forceinline__ double Bv(int m) const { return (double)(float)vs[(ptrdiff_t)m * sl]; }
    __device__ __forceinline__ double R(int m) const { return (double)(float)rho[(ptrdiff_t)m * sl]; }
};

// rayleigh_secular<true> (swd_common.h; surfdisp96.f:773-848) keeping all five components; no water layer.
// mtop: the wavefront's loop bound; a lane with live == false computes on layer 0's values and its e is not read.
__device__ __forceinline__ void rayleigh_vector(double e[5], double wvno, double omga, const ModelGlobal &md, int mmax, int mtop,
                                                bool live, const LibmTabs &LT)
{
    LayerTerms v;
    DivRange dr; // (not read: the divisions are the plain ones)
    dr.reset();
    double omega = omga;
    if (omega < 1.0e-4) omega = 1.0e-4;
    const double wvno2 = wvno * wvno;
    {
        const int mh = live ? mmax - 1 : 0;
        const double ah = md.A(mh), bh = md.Bv(mh);
        const double xka = omega / ah;
        const double xkb = omega / bh;
        double wvnop = wvno + xka;
        double wvnom = fabs(wvno - xka);
        const double ra = sqrt(wvnop * wvnom);
        wvnop = wvno + xkb;
        wvnom = fabs(wvno - xkb);
        const double rb = sqrt(wvnop * wvnom);
        const double t = bh / omega;
        const double gammk = 2.0 * t * t;
        const double gam = gammk * wvno2;
        const double gamm1 = gam - 1.0;
        const double rho1 = md.R(mh);
        e[0] = rho1 * rho1 * (gamm1 * gamm1 - gam * gammk * ra * rb);
        e[1] = -rho1 * ra;
        e[2] = rho1 * (gamm1 - gammk * ra * rb);
        e[3] = rho1 * rb;
        e[4] = wvno2 - ra * rb;
    }
    for (int m = mtop - 2; m >= 0; --m) {
        if (live && m <= mmax - 2) {
            const double am = md.A(m), bm = md.Bv(m);
            const double xka = omega / am;
            const double xkb = omega / bm;
            const double t = bm / omega;
            const double gammk = 2.0 * t * t;
            const double gam = gammk * wvno2;
            double wvnop = wvno + xka;
            double wvnom = fabs(wvno - xka);
            const double ra = sqrt(wvnop * wvnom);
            wvnop = wvno + xkb;
            wvnom = fabs(wvno - xkb);
            const double rb = sqrt(wvnop * wvnom);
            const double dpth = md.D(m);
            const double rho1 = md.R(m);
            const double p = ra * dpth;
            const double q = rb * dpth;
            layer_products(p, q, ra, rb, wvno, xka, xkb, dpth, v, LT);
            Ca19 ca;
            rayleigh_ca19(ca, wvno2, gam, gammk, rho1, v);
            rayleigh_apply<true>(e, ca.c, dr);
        }
    }
}

struct EllipArgs {
    int B, Lmax, K, nsteps;
    const int32_t *nlay;
    const double *h, *vp, *vs, *rho;
    ptrdiff_t sl, sb;
    const double *periods, *vel;
    const int32_t *err;
    double *hv, *mismatch, *cpol;
    int32_t *flag; // zeroed before the launch
    // the fused build (bh_launch_ellip_fused): vel is read with the row stride ldvel; hv is a target's columns of ymod, row stride ldy,
    // and takes y = the transform of include/bh_engine_ellip_target.h; flag is the target's row of err_t, which holds err already
    int ldvel, ldy, zh, is_signed;
    // the site build (EllipFusedArgs::site; include/bh_engine_sites_ellip.h): K is the capacity, periods is not read
    const int32_t *site, *xn;
    const double *xper;
    int nsites, ldn, ldx;
};

// what a lane's pending evaluation is for
enum : int { EL_F0 = 0, EL_F1 = 1, EL_LAST = 2 };

// FUSED: the build of a fused call (bh_launch_ellip_fused).  One statement of the evaluation and the polish for both builds: they
// differ in where a lane reads its velocity and in what `put` does with its result.
template <bool FUSED>
struct EllipOut {
    const EllipArgs &A;
    long long idx, row; // the lane's entry of the [B][K] arrays; of the fused build's output
    bool &flagged;
    // hv (mis, cp: mismatch and cpol where the caller asked for them)
    __device__ __forceinline__ void put(double hv, double mis, double cp) const
    {
        if constexpr (FUSED) {
            double y = A.zh ? 1.0 / hv : hv;
            if (!A.is_signed) y = fabs(y);
            if (!isfinite(y)) { // fails the model in band (SurfEllip.run_models), and the likelihood reads no NaN
                y = 0.0;
                flagged = true;
            }
            A.hv[row] = y;
        } else {
            A.hv[idx] = hv;
            if (A.mismatch) A.mismatch[idx] = mis;
            if (A.cpol) A.cpol[idx] = cp;
        }
    }
};

// SITES (a fused build): a lane reads its model's site's count and its own period from the tables; a lane at or beyond the count --
// count 0, the site lacks the target, included -- or of a site out of range is IDLE: it writes 0.0, raises no flag, evaluates
// nothing and is never live, so neither the wavefront's loop bound nor its ballot sees it.
template <bool FUSED, bool SITES = false>
__global__ __launch_bounds__(ELLIP_THREADS) void swd_ellip_kernel(EllipArgs A)
{
    static_assert(FUSED || !SITES, "the site build is a fused build");
    __shared__ __align__(16) unsigned char smem[ELLIP_LDS];
    const LibmTabs LT = stage_libm_tables(smem, threadIdx.x, ELLIP_THREADS);
    __syncthreads();

    const long long N = (long long)A.B * A.K;
    const long long idx = (long long)blockIdx.x * ELLIP_THREADS + threadIdx.x;
    const bool inrange = idx < N;
    const int b = inrange ? (int)(idx / A.K) : 0;
    const int k = inrange ? (int)(idx % A.K) : 0;
    const int mmax = inrange ? A.nlay[b] : 1;
    const double *periods = A.periods;
    bool idle = false;
    if constexpr (SITES) {
        if (inrange) {
            const int s = A.site[b];
            int n = 0; // (a site out of range reads nothing of the tables)
            if (s >= 0 && s < A.nsites) {
                n = A.xn[(long long)s * A.ldn];
                periods = A.xper + (long long)s * A.ldx;
            }
            idle = k >= n;
            if (idle) A.hv[(long long)b * A.ldy + k] = 0.0;
        }
    }
    const double c = (!inrange || idle) ? 0.0 : FUSED ? A.vel[(long long)b * A.ldvel + k] : A.vel[idx];
    bool flagged = false;
    const EllipOut<FUSED> out{A, idx, (long long)b * A.ldy + k, flagged};
    // no root: nothing is evaluated, the lane's outputs are zero
    bool live = inrange && !idle && A.err[b] == 0 && c > 0.0 && mmax >= 1 && mmax <= A.Lmax;
    if (inrange && !idle && !live) out.put(0.0, 0.0, 0.0);
    ModelGlobal md;
    {
        const ptrdiff_t base = (ptrdiff_t)b * A.sb;
        md.h = A.h + base; md.vp = A.vp + base; md.vs = A.vs + base; md.rho = A.rho + base;
        md.sl = A.sl;
    }
    int mtop = live ? mmax : 1; // the wavefront's largest layer count = the loop bound of the recursion
    for (int off = 32; off > 0; off >>= 1) mtop = max(mtop, __shfl_xor(mtop, off));

    const bool water = live && !((float)md.vs[0] > 0.0f);
    if (water) { // a water layer: not supported, reported in band
        const double qnan = __longlong_as_double(0x7ff8000000000000ll);
        out.put(qnan, qnan, c);
        flagged = true;
        live = false;
    }

    // as SearchT::set_period and the search's rounds form them (swd_common.h, swd_kernel.hip)
    const double twopi = 2.0 * 3.141592653589793;
    const double omega = live ? twopi / periods[k] : 1.0;

    // the polish of the header as a state machine: one evaluation of the compound vector per round for every live lane
    int stage = (A.nsteps == 0) ? EL_LAST : EL_F0;
    int left = A.nsteps;
    double ceval = live ? c : 1.0, c0 = 0.0, f0 = 0.0;
    for (int round = 0; round < A.nsteps + 3; ++round) { // (a bound; the wavefront leaves when its last lane is done)
        if (__ballot(live) == 0ull) break;
        double e[5];
        const double wvno = omega / ceval;
        rayleigh_vector(e, wvno, omega, md, mmax, mtop, live, LT);
        if (!live) continue;
        bool done = false;
        if (stage == EL_F0) {
            c0 = ceval;
            f0 = e[0];
            ceval = c0 * (1.0 + 0x1p-20);
            stage = EL_F1;
        } else if (stage == EL_F1) {
            const double c1 = ceval, f1 = e[0];
            if (left == 0 || f1 == f0) {
                done = true;
            } else {
                const double c2 = c1 - f1 * (c1 - c0) / (f1 - f0);
                if (!(fabs(c2 - c) <= 1.0e-5 * c)) { // the step left the window: the unpolished value
                    ceval = c;
                    flagged = true;
                    stage = EL_LAST;
                } else {
                    c0 = c1;
                    f0 = f1;
                    ceval = c2;
                    --left;
                }
            }
        } else {
            done = true;
        }
        if (done) {
            double hv = e[3] / (wvno * e[2]);
            const double hv_alt = -wvno * e[2] / e[1];
            double mis = fabs(hv - hv_alt) / fabs(hv);
            if (e[1] == 0.0 || e[2] == 0.0 || !isfinite(hv) || !isfinite(hv_alt) || !isfinite(mis)) {
                hv = mis = __longlong_as_double(0x7ff8000000000000ll);
                flagged = true;
            }
            // the gate on the certificate, in every build (the fused ones write no mismatch, but fail the model by it): the two
            // expressions of hv do not agree, so the arithmetic does not determine it; hv, mis and cpol stay as they are
            if (!(mis <= BH_ELLIP_MISMATCH_MAX)) flagged = true;
            out.put(hv, mis, ceval);
            live = false;
        }
    }
    if (flagged) atomicOr(A.flag + b, 1);
}

} // namespace

// The ellipticity target of a fused call (bh_engine.hip: run_forward; bh_device.h), enqueued: nothing is staged or zeroed here
void bh_launch_ellip_fused(const EllipFusedArgs &f, hipStream_t st)
{
    if (f.B <= 0 || f.K <= 0) return;
    EllipArgs a{};
    a.B = f.B; a.Lmax = f.Lmax; a.K = f.K; a.nsteps = f.nsteps;
    a.nlay = f.nlay; a.h = f.h; a.vp = f.vp; a.vs = f.vs; a.rho = f.rho;
    a.sl = f.sl; a.sb = f.sb;
    a.periods = f.periods; a.vel = f.vel; a.err = f.err_row;
    a.hv = f.y; a.flag = f.err_row;
    a.ldvel = f.ldvel; a.ldy = f.ldy; a.zh = f.zh; a.is_signed = f.is_signed;
    const size_t N = (size_t)f.B * (size_t)f.K;
    const dim3 grid((unsigned)((N + ELLIP_THREADS - 1) / ELLIP_THREADS));
    if (f.site != nullptr) { // periods and counts per site (include/bh_engine_sites_ellip.h)
        a.site = f.site; a.nsites = f.nsites; a.xn = f.xn; a.ldn = f.ldn; a.xper = f.xper; a.ldx = f.ldx;
        hipLaunchKernelGGL((swd_ellip_kernel<true, true>), grid, dim3(ELLIP_THREADS), 0, st, a);
        return;
    }
    hipLaunchKernelGGL(swd_ellip_kernel<true>, grid, dim3(ELLIP_THREADS), 0, st, a);
}

extern "C" int bh_swd_ellip(bh_engine *e, int memspace, void *stream, int B, int Lmax, const int32_t *nlay, const double *h,
                            const double *vp, const double *vs, const double *rho, ptrdiff_t sl, ptrdiff_t sb, int K,
                            const double *periods, int have_vel, double *vel, int32_t *err, int nsteps, double *hv, double *mismatch,
                            double *cpol, int32_t *flag)
{
    using namespace bhkit;
    if (!e) return BH_EINVAL;
    if (B < 0 || Lmax < 1 || Lmax > BH_MAX_LAYERS) return fail(e, BH_EINVAL, "bad B or Lmax (1..100)");
    if (sl <= 0 || sb <= 0) return fail(e, BH_EINVAL, "strides must be positive");
    if (K < 1 || K > BH_MAX_PERIODS) return fail(e, BH_EINVAL, "bh_swd_ellip: K must be 1..60");
    if (nsteps < 0 || nsteps > 3) return fail(e, BH_EINVAL, "bh_swd_ellip: nsteps must be 0..3");
    if (!nlay || !h || !vp || !vs || !rho || !periods || !vel || !err || !hv || !flag) return fail(e, BH_EINVAL, "null argument");
    if (B == 0) return BH_OK;
    BH_CHK(e, hipSetDevice(bh_engine_device_internal(e)));
    const bool host = memspace != BH_DEVICE;
    const hipStream_t st = call_stream(e, memspace, stream);
    const size_t N = (size_t)B * (size_t)K;
    const size_t span = ((size_t)(Lmax - 1) * (size_t)sl + (size_t)(B - 1) * (size_t)sb + 1) * sizeof(double);

    EllipArgs a{};
    a.B = B; a.Lmax = Lmax; a.K = K; a.nsteps = nsteps;
    a.sl = sl; a.sb = sb;
    Buf dn, dh, dvp, dvs, drho, dper, dvel, derr, dhv, dmis, dcp, dflag;
    int rc;
    if ((rc = stage(e, st, memspace, nlay, (size_t)B * sizeof(int32_t), dn, &a.nlay))) return rc;
    if ((rc = stage(e, st, memspace, h, span, dh, &a.h))) return rc;
    if ((rc = stage(e, st, memspace, vp, span, dvp, &a.vp))) return rc;
    if ((rc = stage(e, st, memspace, vs, span, dvs, &a.vs))) return rc;
    if ((rc = stage(e, st, memspace, rho, span, drho, &a.rho))) return rc;
    if ((rc = stage(e, st, memspace, periods, (size_t)K * sizeof(double), dper, &a.periods))) return rc;
    double *d_vel = vel;
    int32_t *d_err = err;
    a.hv = hv; a.mismatch = mismatch; a.cpol = cpol; a.flag = flag;
    if (host) {
        if ((rc = alloc(e, dvel, N * sizeof(double)))) return rc;
        if ((rc = alloc(e, derr, (size_t)B * sizeof(int32_t)))) return rc;
        if ((rc = alloc(e, dhv, N * sizeof(double)))) return rc;
        if ((rc = alloc(e, dflag, (size_t)B * sizeof(int32_t)))) return rc;
        if (mismatch && (rc = alloc(e, dmis, N * sizeof(double)))) return rc;
        if (cpol && (rc = alloc(e, dcp, N * sizeof(double)))) return rc;
        d_vel = dvel.as<double>();
        d_err = derr.as<int32_t>();
        a.hv = dhv.as<double>(); a.flag = dflag.as<int32_t>();
        a.mismatch = mismatch ? dmis.as<double>() : nullptr;
        a.cpol = cpol ? dcp.as<double>() : nullptr;
        if (have_vel) {
            BH_CHK(e, hipMemcpyAsync(d_vel, vel, N * sizeof(double), hipMemcpyHostToDevice, st));
            BH_CHK(e, hipMemcpyAsync(d_err, err, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st));
        }
    }
    if (!have_vel) { // the engine's own search, on the same stream (the engine's own for a call of memspace BH_HOST)
        rc = bh_swd_batch(e, BH_DEVICE, (void *)st, B, Lmax, a.nlay, a.h, a.vp, a.vs, a.rho, sl, sb, K, a.periods, BH_WAVE_RAYLEIGH,
                          BH_VEL_PHASE, 1, 0, d_vel, d_err);
        if (rc) {
            if (host) (void)hipStreamSynchronize(st); // (the staging copies read the caller's arrays)
            return rc;
        }
    }
    a.vel = d_vel;
    a.err = d_err;
    BH_CHK(e, hipMemsetAsync(a.flag, 0, (size_t)B * sizeof(int32_t), st));
    const unsigned grid = (unsigned)((N + ELLIP_THREADS - 1) / ELLIP_THREADS);
    hipLaunchKernelGGL(swd_ellip_kernel<false>, dim3(grid), dim3(ELLIP_THREADS), 0, st, a);
    BH_CHK(e, hipGetLastError());
    if (!host) return BH_OK;
    BH_CHK(e, hipMemcpyAsync(hv, a.hv, N * sizeof(double), hipMemcpyDeviceToHost, st));
    if (mismatch) BH_CHK(e, hipMemcpyAsync(mismatch, a.mismatch, N * sizeof(double), hipMemcpyDeviceToHost, st));
    if (cpol) BH_CHK(e, hipMemcpyAsync(cpol, a.cpol, N * sizeof(double), hipMemcpyDeviceToHost, st));
    BH_CHK(e, hipMemcpyAsync(flag, a.flag, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (!have_vel) {
        BH_CHK(e, hipMemcpyAsync(vel, d_vel, N * sizeof(double), hipMemcpyDeviceToHost, st));
        BH_CHK(e, hipMemcpyAsync(err, d_err, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    BH_CHK(e, hipStreamSynchronize(st));
    return BH_OK;
}
