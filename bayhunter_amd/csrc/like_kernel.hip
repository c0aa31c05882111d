// bayhunter_amd/csrc/like_kernel.hip -- noise-covariance laws + Gaussian log-likelihood on gfx950.
//
// Replaces, for a batch of models, the per-target part of JointTarget.evaluate
// (src/Targets.py:322-347): RMS misfit (:99-103), the four covariance laws (:105-173) and
//   logL_t = -1/2 (n ln 2pi + ln|C|) - 1/2 d^T C^-1 d                      (:339-342)
// The reference builds a dense n x n inverse covariance on every call (8 MB at n = 1024);
// here the quadratic forms are evaluated in closed form, O(n) per model:
//   nocorr            Phi = sum d_i^2 / sigma^2
//   nocorr_scalederr  Phi = sum d_i^2 / (s_i sigma^2),  s = yerr/min(yerr) (not squared, as there)
//   exponential       Phi = [(1+r^2) sum d_i^2 - r^2 (d_0^2 + d_{n-1}^2) - 2r sum d_i d_{i+1}]
//                            / (sigma^2 (1-r^2))         (tridiagonal inverse of r^|i-j|)
//   gauss (fixed r)   Phi = d^T R^-1 d / sigma^2, R^-1 constant (host LAPACK, once per chain)
// One 256-thread workgroup per model loops over the targets; wave-level shuffles + LDS for the
// reductions.  HBM traffic: the ymod row of the model (n * 8 B per target).
#include "bh_device.h"
#define BH_HD __device__ __forceinline__
#define BH_TAB static __device__ const
#include "bh_libm.h"
// BH_LIKE_MISSING (like_kernel_m.hip): the builds for sites that lack some of the targets (bh_sites_set_missing,
// include/bh_engine_sites_missing.h) -- the two kernels of the site-count table with a count of 0 skipped -- and their launcher only.
#ifndef BH_LIKE_MISSING
#define BH_LIKE_MISSING 0
#endif
// BH_LIKE_CLASSES (like_kernel_c.hip, on top of BH_LIKE_MISSING): the builds for sites with their own Gauss-law noise correlation
// (bh_sites_set_gauss, include/bh_engine_sites_gauss.h) -- the two kernels of BH_LIKE_MISSING with ln|R| and R^-1 of a Gauss-law
// target from the table of correlation classes -- and their launcher only.
#ifndef BH_LIKE_CLASSES
#define BH_LIKE_CLASSES 0
#endif
// BH_LIKE_LAWS (like_kernel_l.hip, on top of BH_LIKE_CLASSES): the builds for sites with their own noise LAW (bh_sites_set_laws,
// include/bh_engine_sites_laws.h) -- the two kernels of BH_LIKE_CLASSES with every target's law from the table law[site][target] --
// and their launcher only.  A law is uniform over a model's lanes: in the workgroup form one workgroup is one model, so the
// barriers of block_sum that sit under T.law conditions (and those of the in-kernel mat-vec) stay uniform; in the small form one
// wavefront is one model, and that form has no barrier.  The sums s0, s1, sw, d0, dn are formed in the order they have under any
// law and the law only selects among them: a model gets the bits of a launch whose descriptors hold its site's laws.
#ifndef BH_LIKE_LAWS
#define BH_LIKE_LAWS 0
#endif

namespace {

__device__ __forceinline__ double block_sum(double v, double *red)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    __syncthreads();
    if (l == 0) red[w] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// target t of a model of site `site`: that site's observed data (and, law 1, its scaled errors and ln prod of them)
__device__ __forceinline__ LikeTargetDev site_target(LikeTargetDev T, const LikeSiteArgs &S, int site, int ldy, int nt, int t)
{
    T.yobs = S.yobs + (size_t)site * ldy + T.off;
    if (T.law == 1) {
        T.yerr_scaled = S.yerr_scaled + (size_t)site * ldy + T.off;
        T.logdet_extra = S.logdet_extra[(size_t)site * nt + t];
    }
    return T;
}

// ... of a site with its own sample counts (bh_sites_set_x): n from the table -- uniform over the workgroup / wavefront, whose
// model is one -- so the sums below run over the site's first n samples in the order they have for a target of n samples
__device__ __forceinline__ LikeTargetDev site_target(LikeTargetDev T, const LikeSiteXArgs &S, int site, int ldy, int nt, int t)
{
    T = site_target(T, static_cast<const LikeSiteArgs &>(S), site, ldy, nt, t);
    T.n = S.n[(size_t)site * nt + t];
    return T;
}

#if BH_LIKE_CLASSES
// ... of a site with its own noise correlation: a Gauss-law target with a class table takes ln|R| and (the in-kernel mat-vec) R^-1
// of the site's class; a class of -1 goes with a count of 0, and that target is skipped before either is read
__device__ __forceinline__ LikeTargetDev class_target(LikeTargetDev T, const LikeClassArgs &G, int site, int t)
{
    if (T.law == 3 && G.class_of[t] != nullptr) {
        const int c = G.class_of[t][site];
        if (c >= 0) {
            T.logdet_extra = G.logdet[t][c];
            T.rinv = G.rinv[t] + (size_t)c * T.n * T.n;
        }
    }
    return T;
}
#endif

#if BH_LIKE_LAWS
// ... of a site with its own noise law: the law of (site, target) from the table, set BEFORE site_target / class_target so that
// they read the law-1 tables and the class's ln|R| / R^-1 by the site's law (a count of 0 is skipped before the law is used)
__device__ __forceinline__ LikeTargetDev law_target(LikeTargetDev T, const LikeLawArgs &W, int site, int nt, int t)
{
    T.law = W.law[(size_t)site * nt + t];
    return T;
}
#endif

#if !BH_LIKE_MISSING
__global__ __launch_bounds__(256) void like_kernel(LikeKernelArgs A)
{
    constexpr bool SITES = false;
    constexpr LikeSiteArgs S{};
#include "like_body.inc"
}

// the same with a site table (bh_evaluate_sites)
__global__ __launch_bounds__(256) void like_sites_kernel(LikeKernelArgs A, LikeSiteArgs S)
{
    constexpr bool SITES = true;
#include "like_body.inc"
}

// All targets short (n <= 64, e.g. dispersion curves): one WAVEFRONT per model, four models per workgroup, no LDS and
// no barrier -- the workgroup-per-model form above spends most of its 37 us (B = 4096, two targets of 30 periods) in
// two barriers per reduction.  Lane i holds sample i, the sums are the same xor-shuffle tree over the same 64 slots
// (the other three wavefronts of the form above only add zeros): identical bits.
__global__ __launch_bounds__(256) void like_small_kernel(LikeKernelArgs A)
{
    constexpr bool SITES = false;
    constexpr LikeSiteArgs S{};
#include "like_small_body.inc"
}

// the same with a site table (bh_evaluate_sites)
__global__ __launch_bounds__(256) void like_small_sites_kernel(LikeKernelArgs A, LikeSiteArgs S)
{
    constexpr bool SITES = true;
#include "like_small_body.inc"
}

// the site kernels with the sample count of every (site, target) from a table (bh_sites_set_x)
__global__ __launch_bounds__(256) void like_sites_x_kernel(LikeKernelArgs A, LikeSiteXArgs S)
{
    constexpr bool SITES = true;
#include "like_body.inc"
}
__global__ __launch_bounds__(256) void like_small_sites_x_kernel(LikeKernelArgs A, LikeSiteXArgs S)
{
    constexpr bool SITES = true;
#include "like_small_body.inc"
}

__global__ void probe_kernel(int op, int n, const double *in, double *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = (op < 6) ? in[i] : 0.0; // ops >= 6 read their own operands
    double r;
    if (op == 6 || op == 7) { // division probes: in = pairs (a, b)
        const double a = in[2 * i], b = in[2 * i + 1];
        out[i] = (op == 6) ? bh_quot(a, b, bh_rcp_refined(b)) : a / b;
        return;
    }
    if (op >= 8 && op <= 10) { // the glibc-exact exp / sincos of bh_libm.h (tables read from global memory)
        const double v = in[i];
        double sn = 0.0, cs = 0.0;
        if (op == 10) {
            out[i] = bhp_exp_in_domain(v) ? bhp_exp_core(v, bhp_exp_tab) : exp(v);
        } else {
            if (!bhp_sincos_bl(v, &sn, &cs, reinterpret_cast<const double *>(bhp_sincos_tab_bits))) sincos(v, &sn, &cs);
            out[i] = (op == 8) ? sn : cs;
        }
        return;
    }
    switch (op) {
    case 0: r = sqrt(x); break;
    case 1: r = sin(x); break;
    case 2: r = cos(x); break;
    case 3: r = exp(x); break;
    case 4: r = log(x); break;
    default: r = 1.0 / x; break;
    }
    out[i] = r;
}

#elif BH_LIKE_LAWS
__global__ __launch_bounds__(256) void like_sites_l_kernel(LikeKernelArgs A, LikeSiteXArgs S, LikeClassArgs G, LikeLawArgs W)
{
    constexpr bool SITES = true;
#include "like_body.inc"
}
__global__ __launch_bounds__(256) void like_small_sites_l_kernel(LikeKernelArgs A, LikeSiteXArgs S, LikeClassArgs G, LikeLawArgs W)
{
    constexpr bool SITES = true;
#include "like_small_body.inc"
}
#elif BH_LIKE_CLASSES
__global__ __launch_bounds__(256) void like_sites_c_kernel(LikeKernelArgs A, LikeSiteXArgs S, LikeClassArgs G)
{
    constexpr bool SITES = true;
#include "like_body.inc"
}
__global__ __launch_bounds__(256) void like_small_sites_c_kernel(LikeKernelArgs A, LikeSiteXArgs S, LikeClassArgs G)
{
    constexpr bool SITES = true;
#include "like_small_body.inc"
}
#else
// the kernels of the site-count table where a count may be 0: that target is skipped (like_body.inc, like_small_body.inc)
__global__ __launch_bounds__(256) void like_sites_m_kernel(LikeKernelArgs A, LikeSiteXArgs S)
{
    constexpr bool SITES = true;
#include "like_body.inc"
}
__global__ __launch_bounds__(256) void like_small_sites_m_kernel(LikeKernelArgs A, LikeSiteXArgs S)
{
    constexpr bool SITES = true;
#include "like_small_body.inc"
}
#endif

} // namespace

#if BH_LIKE_LAWS
void bh_launch_like_sites_l(const LikeKernelArgs &a, const LikeSiteXArgs &sites, const LikeClassArgs &classes, const LikeLawArgs &laws,
                            hipStream_t stream)
{
    size_t lds = 0;
    const bool small = bh_like_small_form(a, &lds); // (by the descriptors: a Gauss-law descriptor owns the contraction's workspace and the LDS)
    if (small) hipLaunchKernelGGL(like_small_sites_l_kernel, dim3((a.B + 3) / 4), dim3(256), 0, stream, a, sites, classes, laws);
    else hipLaunchKernelGGL(like_sites_l_kernel, dim3(a.B), dim3(256), lds, stream, a, sites, classes, laws);
}
#elif BH_LIKE_CLASSES
void bh_launch_like_sites_c(const LikeKernelArgs &a, const LikeSiteXArgs &sites, const LikeClassArgs &classes, hipStream_t stream)
{
    size_t lds = 0;
    const bool small = bh_like_small_form(a, &lds);
    if (small) hipLaunchKernelGGL(like_small_sites_c_kernel, dim3((a.B + 3) / 4), dim3(256), 0, stream, a, sites, classes);
    else hipLaunchKernelGGL(like_sites_c_kernel, dim3(a.B), dim3(256), lds, stream, a, sites, classes);
}
#elif BH_LIKE_MISSING
void bh_launch_like_sites_m(const LikeKernelArgs &a, const LikeSiteXArgs &sites, hipStream_t stream)
{
    size_t lds = 0;
    const bool small = bh_like_small_form(a, &lds);
    if (small) hipLaunchKernelGGL(like_small_sites_m_kernel, dim3((a.B + 3) / 4), dim3(256), 0, stream, a, sites);
    else hipLaunchKernelGGL(like_sites_m_kernel, dim3(a.B), dim3(256), lds, stream, a, sites);
}
#else
static void launch_like(const LikeKernelArgs &a, const LikeSiteArgs *sites, hipStream_t stream, const LikeSiteXArgs *sx = nullptr)
{
    size_t lds = 0;
    const bool small = bh_like_small_form(a, &lds); // (bh_device.h: shared with like_kernel_m.hip)
    if (sx != nullptr) { // (n = the capacity of the target's columns: a site's own count is at most that)
        if (small) hipLaunchKernelGGL(like_small_sites_x_kernel, dim3((a.B + 3) / 4), dim3(256), 0, stream, a, *sx);
        else hipLaunchKernelGGL(like_sites_x_kernel, dim3(a.B), dim3(256), lds, stream, a, *sx);
        return;
    }
    if (sites != nullptr) {
        if (small) hipLaunchKernelGGL(like_small_sites_kernel, dim3((a.B + 3) / 4), dim3(256), 0, stream, a, *sites);
        else hipLaunchKernelGGL(like_sites_kernel, dim3(a.B), dim3(256), lds, stream, a, *sites);
        return;
    }
    if (small) hipLaunchKernelGGL(like_small_kernel, dim3((a.B + 3) / 4), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(like_kernel, dim3(a.B), dim3(256), lds, stream, a);
}

void bh_launch_like(const LikeKernelArgs &a, hipStream_t stream) { launch_like(a, nullptr, stream); }
void bh_launch_like_sites(const LikeKernelArgs &a, const LikeSiteArgs &sites, hipStream_t stream) { launch_like(a, &sites, stream); }
void bh_launch_like_sites_x(const LikeKernelArgs &a, const LikeSiteXArgs &sites, hipStream_t stream) { launch_like(a, nullptr, stream, &sites); }

void bh_launch_probe(int op, int n, const double *in, double *out, hipStream_t stream)
{
    hipLaunchKernelGGL(probe_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, op, n, in, out);
}
#endif
