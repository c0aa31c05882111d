// bayhunter_amd/csrc/posterior_cov_kernel.hip -- posterior covariance and correlation of vs with depth (include/bh_engine_posterior_cov.h).
//
// P = D + Qc columns per site: the vs of a row at D depths (posterior_kernel.hip's sampling) and Qc columns of a scalar set.
//   mask     : one lane per row: NaN in any chosen scalar column leaves the row out of the whole matrix (listwise deletion)
//   stats    : a wavefront is 64 columns of one site over a chunk of its rows: min, max and the lowest set bit of the rows used
//   contract : V^T V on the FP64 matrix cores.  A workgroup (4 wavefronts) takes one chunk and one group of 4 x 4 tiles of
//              16 x 16 of the upper triangle: 64 columns down (side 0) by 64 columns across (side 1; the same 64 on the diagonal).
//              Per step of COV_ROWS rows wavefront w forms the rows w, w + 4, .. of both sides, a lane per column: Y = rint(v 2^-L)
//              - X0 as two 14-bit limbs, as doubles, into LDS; a masked row and a column or row past the end give zero limbs.  Then
//              wavefront w accumulates tile row w of the group: per tile and 4 rows four v_mfma_f64_16x16x4_f64 -- H.H, H.Lo and
//              Lo.H into one accumulator, Lo.Lo.  At the end of the chunk the accumulators are converted to integers (exact) and
//              meet the other chunks in 64-bit integer atomics; so do the column sums.  No floating-point atomics anywhere.
// The finished numbers are formed on the host with 128-bit integers (bh_posterior_cov_finish).
#include "posterior_select.h"
#include "../../include/bh_engine_posterior_cov.h"
#include "../../include/bh_engine_posterior_features.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#define COV_ROWS 16   // rows per step of the contraction (a multiple of 4, the k of one MFMA, and of the 4 wavefronts)
#define COV_SIDE 64   // columns per side of a tile group: 4 tiles of 16
#define COV_LD 80     // doubles per LDS row: 64 + 16, so that the rows k and k + 1 a half-wavefront reads lie in different banks

// Exactness of the contraction.  Limbs are below 2^BH_COV_LIMB_BITS, so a product is below 2^28 and the middle accumulator
// (H.Lo + Lo.H) takes below 2^29 per row; a chunk has at most POST_CHUNK = 2^13 rows: every partial sum is an integer below 2^42,
// far below 2^53 -- float64 adds them exactly in whatever order the matrix core takes them.
static_assert(2 * BH_COV_LIMB_BITS == 28, "Y < 2^28 is two limbs");
static_assert((unsigned long long)POST_CHUNK * (2ull << (2 * BH_COV_LIMB_BITS)) <= (1ull << 53),
              "a chunk's partial sums must stay exact integers in float64");
static_assert(COV_ROWS % 4 == 0 && BH_COV_MAXCOLS % COV_SIDE == 0, "whole MFMA steps, whole tile groups");

using namespace bhpost;

namespace {

typedef double cov_d4 __attribute__((ext_vector_type(4)));

struct CovArgs {
    const PostWork *work;
    const int32_t *pn;
    const void *pvs;
    const double *pd;
    int ML, D, P;
    const double *dep;          // [D]
    const double *val;          // the set's table val[q * nrows + r] (Qc > 0)
    const int32_t *cols;        // [Qc]: the chosen columns of the set
    int64_t nrows;
    const unsigned char *mask;  // [nrows]: 1 = the row is left out (Qc > 0), else null
};

// vs of a row at depth x: vs[#{j : d_j <= x}] (posterior_kernel.hip's sample)
template <typename T>
__device__ __forceinline__ double cov_sample(int n, const T *vs, const double *d, double x)
{
    int k = 0;
    for (int j = 0; j < n - 1; ++j) k += d[j] <= x ? 1 : 0;
    double v = (double)vs[0];
    for (int j = 1; j < n; ++j) v = k == j ? (double)vs[j] : v;
    return v;
}

// a lane's column: 0 = past the end, 1 = vs at depth x, 2 = the scalar column at col
struct CovCol {
    int kind;
    double x;
    const double *col;
};

__device__ __forceinline__ CovCol cov_col(const CovArgs &a, int j)
{
    CovCol c;
    c.kind = j < a.D ? 1 : j < a.P ? 2 : 0;
    c.x = c.kind == 1 ? a.dep[j] : 0.0;
    c.col = c.kind == 2 ? a.val + (int64_t)a.cols[j - a.D] * a.nrows : nullptr;
    return c;
}

template <typename T>
__device__ __forceinline__ double cov_value(const CovArgs &a, const CovCol &c, int64_t r)
{
    if (c.kind == 1) return cov_sample(a.pn[r], (const T *)a.pvs + r * a.ML, a.pd + r * a.ML, c.x);
    return c.kind == 2 ? c.col[r] : 0.0;
}

__global__ void __launch_bounds__(256) cov_mask_kernel(int64_t nrows, const int32_t *psite, const double *val, const int32_t *cols,
                                                       int Qc, unsigned char *mask, unsigned long long *nmasked)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool m = false;
    int s = 0;
    if (r < nrows) {
        s = psite[r];
        for (int q = 0; q < Qc; ++q) {
            const double v = val[(int64_t)cols[q] * nrows + r];
            m = m || v != v;
        }
        mask[r] = m ? 1 : 0;
    }
    agg_add(nmasked, s, m);
}

template <typename T>
__global__ void __launch_bounds__(64) cov_stats_kernel(CovArgs a, unsigned long long *kmin, unsigned long long *kmax, int *low)
{
    const PostWork w = a.work[blockIdx.x];
    const int j = blockIdx.y * 64 + threadIdx.x;
    const CovCol c = cov_col(a, j);
    unsigned long long mn = ~0ull, mx = 0;
    int lo = INT_MAX;
    for (int64_t r = w.r0; r < w.r1; ++r) {
        if (a.mask && a.mask[r]) continue; // (uniform)
        const double v = cov_value<T>(a, c, r);
        const unsigned long long k = okey(v, false);
        mn = k < mn ? k : mn;
        mx = k > mx ? k : mx;
        const int b = low_bit(v);
        lo = b < lo ? b : lo;
    }
    if (!c.kind || mn > mx) return; // past the end, or no row of the chunk is used
    const size_t o = (size_t)w.site * a.P + j;
    atomicMin(&kmin[o], mn);
    atomicMax(&kmax[o], mx);
    atomicMin(&low[o], lo);
}

typedef double CovLimbs[2][COV_ROWS][COV_LD]; // of one side: [H, Lo][row of the step][column of the side]

// One chunk against the group (bi, bj) whose side 1 has NT tile columns inside P -- the same NT for the whole workgroup.  The
// accumulators of a wavefront are NT tiles x 3 x 8 registers; every MFMA is issued unconditionally (on the diagonal group the tiles
// below the diagonal are computed and not written: the wavefronts meet at the barriers of every step, so the step takes as long as
// the wavefront of the first tile row either way).
template <typename T, int NT>
__device__ __forceinline__ void cov_body(const CovArgs &a, const PostWork &w, int bi, int bj, const int32_t *scale, const int64_t *x0,
                                         unsigned long long *s, unsigned long long *raw, CovLimbs *lim)
{
    const bool diag = bi == bj;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int fi = lane & 15, fk = lane >> 4;

    // the lane's column of either side, with its scale and offset
    const int gc[2] = {bi * COV_SIDE + lane, bj * COV_SIDE + lane};
    CovCol cc[2];
    int L[2];
    long long X0[2];
#pragma unroll
    for (int sd = 0; sd < 2; ++sd) {
        cc[sd] = cov_col(a, gc[sd]);
        const size_t o = (size_t)w.site * a.P + (cc[sd].kind ? gc[sd] : 0);
        L[sd] = cc[sd].kind ? scale[o] : 0;
        X0[sd] = cc[sd].kind ? (long long)x0[o] : 0;
    }
    const int ti = 4 * bi + wave; // the wavefront's tile row, against the tile columns 4 bj + 0 .. NT - 1
    cov_d4 c0[NT], c1[NT], c2[NT];
#pragma unroll
    for (int jt = 0; jt < NT; ++jt) c0[jt] = c1[jt] = c2[jt] = (cov_d4){0.0, 0.0, 0.0, 0.0};
    const CovLimbs &A = lim[0], &B = lim[diag ? 0 : 1];
    unsigned long long ssum = 0;

    for (int64_t rb = w.r0; rb < w.r1; rb += COV_ROWS) {
#pragma unroll 1
        for (int i = 0; i < COV_ROWS / 4; ++i) {
            const int rr = wave + 4 * i;
            const int64_t r = rb + rr;
            const bool live = r < w.r1 && !(a.mask && a.mask[r]); // (uniform over the wavefront)
#pragma unroll
            for (int sd = 0; sd < 2; ++sd) {
                if (sd && diag) continue;
                long long Y = 0;
                if (live && cc[sd].kind) Y = (long long)rint(ldexp(cov_value<T>(a, cc[sd], r), -L[sd])) - X0[sd];
                lim[sd][0][rr][lane] = (double)(Y >> BH_COV_LIMB_BITS);
                lim[sd][1][rr][lane] = (double)(Y & ((1ll << BH_COV_LIMB_BITS) - 1));
                if (sd == 0) ssum += (unsigned long long)Y;
            }
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < COV_ROWS; kk += 4) {
            // A[i = fi][k = fk] and B[k = fk][j = fi]: one f64 per lane each
            const double ah = A[0][kk + fk][16 * wave + fi], al = A[1][kk + fk][16 * wave + fi];
#pragma unroll
            for (int jt = 0; jt < NT; ++jt) {
                const double bh = B[0][kk + fk][16 * jt + fi], bl = B[1][kk + fk][16 * jt + fi];
                c0[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(ah, bh, c0[jt], 0, 0, 0);
                c1[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(ah, bl, c1[jt], 0, 0, 0);
                c1[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(al, bh, c1[jt], 0, 0, 0);
                c2[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(al, bl, c2[jt], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // c[jt][reg] = the sums of column i = 16 ti + fk + 4 reg against column j = 16 (4 bj + jt) + fi; written where i <= j < P
    const size_t npair = (size_t)a.P * (a.P + 1) / 2;
    unsigned long long *out = raw + (size_t)w.site * npair * 3;
#pragma unroll
    for (int jt = 0; jt < NT; ++jt) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int i = 16 * ti + fk + 4 * reg, j = 16 * (4 * bj + jt) + fi;
            if (i > j || j >= a.P) continue;
            unsigned long long *o = out + ((size_t)i * a.P - (size_t)i * (i - 1) / 2 + (size_t)(j - i)) * 3;
            const unsigned long long v0 = (unsigned long long)c0[jt][reg], v1 = (unsigned long long)c1[jt][reg],
                                     v2 = (unsigned long long)c2[jt][reg];
            if (v0) atomicAdd(&o[0], v0);
            if (v1) atomicAdd(&o[1], v1);
            if (v2) atomicAdd(&o[2], v2);
        }
    }
    // the column sums, once per column: from the diagonal groups, every wavefront its rows
    if (diag && cc[0].kind && ssum) atomicAdd(&s[(size_t)w.site * a.P + gc[0]], ssum);
}

// raw[site][pair(i, j)][3], i <= j row-major; s[site][P].  grid: (chunks, groups = the blocks (bi, bj), bi <= bj, of COV_SIDE columns)
template <typename T>
__global__ void __launch_bounds__(256) cov_contract_kernel(CovArgs a, const int32_t *scale, const int64_t *x0,
                                                           unsigned long long *s, unsigned long long *raw)
{
    __shared__ CovLimbs lim[2];
    const PostWork w = a.work[blockIdx.x];
    const int nb = (a.P + COV_SIDE - 1) / COV_SIDE;
    int g = blockIdx.y, bi = 0;
    while (g >= nb - bi) { g -= nb - bi; ++bi; }
    const int bj = bi + g;
    const int nt = (a.P - bj * COV_SIDE + 15) / 16; // the tile columns of side 1 inside P: 1 .. 4 in the last block, 4 before it
    if (nt >= 4) cov_body<T, 4>(a, w, bi, bj, scale, x0, s, raw, lim);
    else if (nt == 3) cov_body<T, 3>(a, w, bi, bj, scale, x0, s, raw, lim);
    else if (nt == 2) cov_body<T, 2>(a, w, bi, bj, scale, x0, s, raw, lim);
    else cov_body<T, 1>(a, w, bi, bj, scale, x0, s, raw, lim);
}

// ---- host side ---------------------------------------------------------------------------------------------------

// rint(mx 2^-L) - rint(mn 2^-L) < 2^28 (both integers of at most 53 bits where L is at or above the lowest set bit: the difference
// may round, never across 2^28)
bool cov_fits(double mn, double mx, int L)
{
    return std::nearbyint(std::ldexp(mx, -L)) - std::nearbyint(std::ldexp(mn, -L)) < 268435456.0;
}

// the smallest L >= low that fits (the width shrinks as L grows: the first that fits going up)
int cov_scale(double mn, double mx, int low)
{
    int L = low;
    if (cov_fits(mn, mx, L)) return L;
    int e;
    (void)std::frexp(mx / 2 - mn / 2, &e); // mx - mn >= 2^(e - 1) (1 - 2^-52): nothing below e - 31 fits
    L = std::max(low, e - 31);
    while (!cov_fits(mn, mx, L)) ++L;
    return L;
}

typedef __int128 cov_i128;

long double cov_ld(cov_i128 v) // to 64 bits of mantissa, one rounding
{
    const bool neg = v < 0;
    const unsigned __int128 u = neg ? (unsigned __int128)(-v) : (unsigned __int128)v;
    const long double r = std::ldexp((long double)(uint64_t)(u >> 64), 64) + (long double)(uint64_t)u;
    return neg ? -r : r;
}

} // namespace

extern "C" {

int bh_posterior_cov_finish(int nsites, int P, const int64_t *n, const int32_t *L, const int64_t *x0, const uint64_t *s,
                            const uint64_t *raw, double *mean, double *cov, double *corr)
{
    if (nsites < 1 || P < 1 || P > BH_COV_MAXCOLS || !n || !L || !x0 || !s || !raw) return BH_EINVAL;
    for (int t = 0; t < nsites; ++t) {
        if (n[t] < 0) return BH_EINVAL;
        if (n[t] > (int64_t)BH_COV_MAXROWS) return BH_EUNSUPPORTED;
    }
    const size_t npair = (size_t)P * (P + 1) / 2;
    const double nan = std::nan("");
    std::vector<cov_i128> N(npair);
    for (int t = 0; t < nsites; ++t) {
        const int64_t nn = n[t];
        const int32_t *Ls = L + (size_t)t * P;
        const int64_t *xs = x0 + (size_t)t * P;
        const uint64_t *ss = s + (size_t)t * P, *rs = raw + (size_t)t * npair * 3;
        double *m = mean ? mean + (size_t)t * P : nullptr;
        double *cv = cov ? cov + (size_t)t * P * P : nullptr, *cr = corr ? corr + (size_t)t * P * P : nullptr;
        if (nn == 0) {
            for (int i = 0; m && i < P; ++i) m[i] = nan;
            for (size_t i = 0; i < (size_t)P * P; ++i) {
                if (cv) cv[i] = nan;
                if (cr) cr[i] = nan;
            }
            continue;
        }
        // N_ij = n S_ij - s_i s_j, S_ij = raw0 2^28 + raw1 2^14 + raw2
        size_t q = 0;
        for (int i = 0; i < P; ++i)
            for (int j = i; j < P; ++j, ++q) {
                const cov_i128 S = ((cov_i128)rs[3 * q] << (2 * BH_COV_LIMB_BITS)) + ((cov_i128)rs[3 * q + 1] << BH_COV_LIMB_BITS) +
                                   (cov_i128)rs[3 * q + 2];
                N[q] = (cov_i128)nn * S - (cov_i128)ss[i] * (cov_i128)ss[j];
            }
        const long double n2 = (long double)nn * (long double)nn; // < 2^48: exact
        for (int i = 0; m && i < P; ++i)
            m[i] = (double)std::ldexp(cov_ld((cov_i128)ss[i] + (cov_i128)nn * (cov_i128)xs[i]) / (long double)nn, Ls[i]);
        q = 0;
        for (int i = 0; i < P; ++i) {
            const cov_i128 Nii = N[(size_t)i * P - (size_t)i * (i - 1) / 2];
            for (int j = i; j < P; ++j, ++q) {
                const cov_i128 Njj = N[(size_t)j * P - (size_t)j * (j - 1) / 2];
                if (cv) cv[(size_t)i * P + j] = cv[(size_t)j * P + i] = (double)std::ldexp(cov_ld(N[q]) / n2, Ls[i] + Ls[j]);
                if (cr) {
                    double v;
                    if (Nii <= 0 || Njj <= 0) v = nan;
                    else if (i == j) v = 1.0;
                    else v = std::min(1.0, std::max(-1.0, (double)(cov_ld(N[q]) / std::sqrt(cov_ld(Nii) * cov_ld(Njj)))));
                    cr[(size_t)i * P + j] = cr[(size_t)j * P + i] = v;
                }
            }
        }
    }
    return BH_OK;
}

int bh_posterior_cov(bh_posterior *p, int D, const double *dep, int set, int Qc, const int32_t *cols, int64_t *n_out,
                     int64_t *masked_out, int32_t *L_out, int64_t *x0_out, int32_t *exact_out, uint64_t *s_out, uint64_t *raw_out,
                     double *mean, double *cov, double *corr)
{
    int rc;
    if (!p) return BH_EINVAL;
    if (p->S < 1) return pfail(p, BH_EINVAL, "no rows loaded (bh_posterior_load)");
    if (D < 0 || Qc < 0 || D + Qc < 1 || D > BH_COV_MAXCOLS || Qc > BH_COV_MAXCOLS || D + Qc > BH_COV_MAXCOLS)
        return pfail(p, BH_EINVAL, "columns: 1 <= D + Qc <= BH_COV_MAXCOLS (256)");
    if ((D && !dep) || (Qc && !cols)) return pfail(p, BH_EINVAL, "null argument");
    for (int j = 0; j < D; ++j)
        if (!std::isfinite(dep[j]) || (j && !(dep[j] > dep[j - 1])))
            return pfail(p, BH_EINVAL, "depth grid must be finite and strictly ascending");
    const ScalarSet *ss = nullptr;
    if (Qc) {
        if (set != BH_SCALARS_MOHO && set != BH_SCALARS_USER && set != BH_SCALARS_FEATURES)
            return pfail(p, BH_EINVAL, "scalar columns come from BH_SCALARS_MOHO or BH_SCALARS_USER (or BH_SCALARS_FEATURES)");
        if (!p->has_rows) return pfail(p, BH_EINVAL, "the rows were loaded without bh_posterior_keep_rows");
        ss = &p->sets[set_slot(set)];
        if (ss->Q < 1)
            return pfail(p, BH_EINVAL, set == BH_SCALARS_MOHO   ? "the MOHO set does not exist yet (bh_posterior_moho)"
                                       : set == BH_SCALARS_USER ? "the USER set does not exist yet (bh_posterior_attach)"
                                                                : "the FEATURES set does not exist yet (bh_posterior_features)");
        for (int q = 0; q < Qc; ++q)
            if (cols[q] < 0 || cols[q] >= ss->Q) return pfail(p, BH_EINVAL, "column out of range");
    } else if (set != -1 && set != BH_SCALARS_MOHO && set != BH_SCALARS_USER && set != BH_SCALARS_FEATURES) {
        return pfail(p, BH_EINVAL, "no such scalar set");
    }
    const int S = p->S, P = D + Qc;
    const size_t npair = (size_t)P * (P + 1) / 2;
    if ((size_t)S * npair > (size_t)BH_COV_MAXCELLS)
        return pfail(p, BH_EINVAL, "nsites * P (P + 1) / 2 would exceed BH_COV_MAXCELLS (2^24) cells");
    for (int t = 0; t < S; ++t)
        if (p->off[t + 1] - p->off[t] > (int64_t)BH_COV_MAXROWS) return pfail(p, BH_EUNSUPPORTED, "2^24 or more rows of one site");
    PCHK(p, hipSetDevice(p->device));
    const size_t ncol = (size_t)S * P;
    Dev dd, dcols, dmask, dnm, dmin, dmax, dlow, dsc, dx0, ds, draw;
    if ((rc = alloc(p, dd, (size_t)D * 8)) || (rc = alloc(p, dcols, (size_t)Qc * 4)) || (rc = alloc(p, dnm, (size_t)S * 8)) ||
        (rc = alloc(p, dmin, ncol * 8)) || (rc = alloc(p, dmax, ncol * 8)) || (rc = alloc(p, dlow, ncol * 4)) ||
        (rc = alloc(p, dsc, ncol * 4)) || (rc = alloc(p, dx0, ncol * 8)) || (rc = alloc(p, ds, ncol * 8)) ||
        (rc = alloc(p, draw, (size_t)S * npair * 24)))
        return rc;
    if (Qc && (rc = alloc(p, dmask, (size_t)p->nrows))) return rc;
    if (D) PCHK(p, hipMemcpyAsync(dd.p, dep, (size_t)D * 8, hipMemcpyHostToDevice, p->st));
    if (Qc) PCHK(p, hipMemcpyAsync(dcols.p, cols, (size_t)Qc * 4, hipMemcpyHostToDevice, p->st));
    PCHK(p, hipMemsetAsync(dnm.p, 0, (size_t)S * 8, p->st));
    PCHK(p, hipMemsetAsync(dmin.p, 0xff, ncol * 8, p->st));
    PCHK(p, hipMemsetAsync(dmax.p, 0, ncol * 8, p->st));
    PCHK(p, hipMemsetAsync(dlow.p, 0x7f, ncol * 4, p->st)); // 0x7f7f7f7f: above every exponent
    PCHK(p, hipMemsetAsync(ds.p, 0, ncol * 8, p->st));
    PCHK(p, hipMemsetAsync(draw.p, 0, (size_t)S * npair * 24, p->st));
    CovArgs a;
    a.work = p->dwork.as<PostWork>();
    a.pn = p->pn.as<int32_t>();
    a.pvs = p->pvs.p;
    a.pd = p->pd.as<double>();
    a.ML = p->ML;
    a.D = D;
    a.P = P;
    a.dep = dd.as<double>();
    a.val = Qc ? ss->val.as<double>() : nullptr;
    a.cols = dcols.as<int32_t>();
    a.nrows = p->nrows;
    a.mask = Qc ? dmask.as<unsigned char>() : nullptr;
    const bool f = p->elem == 4, any = !p->work.empty();
    if (Qc && p->nrows) {
        cov_mask_kernel<<<(unsigned)((p->nrows + 255) / 256), 256, 0, p->st>>>(p->nrows, p->psite.as<int32_t>(), a.val, a.cols, Qc,
                                                                               dmask.as<unsigned char>(), dnm.as<unsigned long long>());
        PCHK(p, hipGetLastError());
    }
    if (any) {
        const dim3 grid((unsigned)p->work.size(), (unsigned)((P + 63) / 64));
        if (f) cov_stats_kernel<float><<<grid, 64, 0, p->st>>>(a, dmin.as<unsigned long long>(), dmax.as<unsigned long long>(), dlow.as<int>());
        else cov_stats_kernel<double><<<grid, 64, 0, p->st>>>(a, dmin.as<unsigned long long>(), dmax.as<unsigned long long>(), dlow.as<int>());
        PCHK(p, hipGetLastError());
    }
    std::vector<unsigned long long> nm(S);
    std::vector<uint64_t> kmin(ncol), kmax(ncol), hs(ncol), hraw((size_t)S * npair * 3);
    std::vector<int32_t> low(ncol), Lh(ncol), ex(ncol);
    std::vector<int64_t> xh(ncol), nh(S);
    PCHK(p, hipMemcpyAsync(nm.data(), dnm.p, (size_t)S * 8, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipMemcpyAsync(kmin.data(), dmin.p, ncol * 8, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipMemcpyAsync(kmax.data(), dmax.p, ncol * 8, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipMemcpyAsync(low.data(), dlow.p, ncol * 4, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipStreamSynchronize(p->st));
    for (int t = 0; t < S; ++t) nh[t] = p->off[t + 1] - p->off[t] - (int64_t)nm[t];
    for (size_t c = 0; c < ncol; ++c) {
        Lh[c] = 0;
        xh[c] = 0;
        ex[c] = 1;
        if (nh[c / P] == 0) continue;
        const double vmn = okey64_value(kmin[c]), vmx = okey64_value(kmax[c]);
        if (!std::isfinite(vmn) || !std::isfinite(vmx))
            return pfail(p, BH_EINVAL, c % P < (size_t)D ? "a velocity is not finite" : "a value of a scalar column is not finite");
        if (vmn == 0.0 && vmx == 0.0) continue; // zeros only (no set bit: low is still what the memset left)
        Lh[c] = cov_scale(vmn, vmx, low[c]);
        ex[c] = Lh[c] == low[c];
        xh[c] = (int64_t)std::nearbyint(std::ldexp(vmn, -Lh[c]));
    }
    PCHK(p, hipMemcpyAsync(dsc.p, Lh.data(), ncol * 4, hipMemcpyHostToDevice, p->st));
    PCHK(p, hipMemcpyAsync(dx0.p, xh.data(), ncol * 8, hipMemcpyHostToDevice, p->st));
    if (any) {
        const int nb = (P + COV_SIDE - 1) / COV_SIDE;
        const dim3 grid((unsigned)p->work.size(), (unsigned)(nb * (nb + 1) / 2));
        if (f) cov_contract_kernel<float><<<grid, 256, 0, p->st>>>(a, dsc.as<int32_t>(), dx0.as<int64_t>(), ds.as<unsigned long long>(), draw.as<unsigned long long>());
        else cov_contract_kernel<double><<<grid, 256, 0, p->st>>>(a, dsc.as<int32_t>(), dx0.as<int64_t>(), ds.as<unsigned long long>(), draw.as<unsigned long long>());
        PCHK(p, hipGetLastError());
    }
    PCHK(p, hipMemcpyAsync(hs.data(), ds.p, ncol * 8, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipMemcpyAsync(hraw.data(), draw.p, (size_t)S * npair * 24, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipStreamSynchronize(p->st));
    // everything is here: only now the caller's buffers are written
    for (int t = 0; t < S; ++t) {
        if (n_out) n_out[t] = nh[t];
        if (masked_out) masked_out[t] = (int64_t)nm[t];
    }
    if (L_out) std::memcpy(L_out, Lh.data(), ncol * 4);
    if (x0_out) std::memcpy(x0_out, xh.data(), ncol * 8);
    if (exact_out) std::memcpy(exact_out, ex.data(), ncol * 4);
    if (s_out) std::memcpy(s_out, hs.data(), ncol * 8);
    if (raw_out) std::memcpy(raw_out, hraw.data(), (size_t)S * npair * 24);
    if ((rc = bh_posterior_cov_finish(S, P, nh.data(), Lh.data(), xh.data(), hs.data(), hraw.data(), mean, cov, corr)))
        return pfail(p, rc, "bh_posterior_cov_finish refused the sums");
    return BH_OK;
}

} // extern "C"
