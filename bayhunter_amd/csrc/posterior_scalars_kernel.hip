// bayhunter_amd/csrc/posterior_scalars_kernel.hip -- per-site posteriors of scalar columns (include/bh_engine_posterior_scalars.h).
//
// A scalar set is a table val[q][row] of float64 over the rows bh_posterior_load left grouped by site (NaN = no value).
//   moho    : one lane per row applies the Moho rule to the row's vs, zd and step-model depths and writes its four columns
//   attach  : one lane per row gathers the caller's value row by the row's index in the loaded input (+ nlayers = n - 1)
// The passes over a set: a workgroup is (chunk of at most POST_CHUNK rows of one site, column), a lane per row, strided.
// Lanes reduce in registers, wavefronts by shuffles, and chunks meet in integer atomics only (counts, min / max of
// ordered keys, 64-bit limb sums), so a site's results are the same bits in every run, alone or among other sites.
//   stats   : count, NaN count, min, max, lowest set bit, float32-exactness of every (site, column)
//   moments : the 32-bit limbs of sum(Y) and sum(Y^2), Y = v * 2^-scale - X0 (posterior_kernel.hip's encoding)
//   radix   : the median by the radix select of posterior_select.h on the ordered key, 8 bits per pass, 256 LDS counters; a column of
//             float32-exact values has 32-bit keys (4 passes).  A last pass finds the next key above the selected one.
//   hist    : numpy.histogram over per-site edges; edges and counters in LDS where a site has at most SC_LDS_BINS bins
//   hist2d  : numpy.histogram2d of one column against another; in LDS where a site has at most SC_LDS_CELLS cells
// LDS: 24 KiB (hist), 32 KiB (hist2d), 1 KiB (radix) per 256-lane workgroup -- several workgroups per CU beside each other.
// -ffp-contract=off (Makefile): no product of the crustal mean is contracted into its sum.
#include "posterior_select.h"
#include "../../include/bh_engine_posterior_datafit.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#define SC_THREADS 256
#define SC_LDS_BINS 2048    // 1-D: 8 KiB of counters + 16 KiB of edges
#define SC_LDS_CELLS 4096   // 2-D: 16 KiB of counters
#define SC_LDS_EDGES 2048   // 2-D: nx + ny + 2 edges, 16 KiB

using namespace bhpost;

namespace {

// (double)vs_j * h_j of a row, h_j = (double)zd_j - (double)zd_{j-1}
template <typename T>
__device__ __forceinline__ double crust_term(const T *vs, const T *zd, int j)
{
    const double h = (double)zd[j] - (j ? (double)zd[j - 1] : 0.0);
    return (double)vs[j] * h;
}

// one lane per loaded row: the Moho rule (header); val[c * nrows + r], c = moho, vslast, vscrust, vsjump
template <typename T>
__global__ void __launch_bounds__(256) sc_moho_kernel(int64_t nrows, int ML, const int32_t *pn, const int32_t *psite,
                                                      const T *pvs, const T *pzd, const double *pd, const double *lo,
                                                      const double *hi, const double *mohovs, double *val,
                                                      unsigned long long *found)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int k = -1, s = 0;
    if (r < nrows) {
        s = psite[r];
        const int n = pn[r];
        const T *vs = pvs + r * ML, *zd = pzd + r * ML;
        const double *d = pd + r * ML;
        const double l = lo[s], h = hi[s], mv = mohovs[s];
        for (int j = n - 2; j >= 0; --j) k = (d[j] > l && d[j] < h && (double)vs[j + 1] > mv) ? j : k;
        double moho = qnan(), last = qnan(), crust = qnan(), jump = qnan();
        if (k >= 0) {
            const int m = k + 1;
            double sum;
            if (m < 8) {
                sum = crust_term(vs, zd, 0);
                for (int j = 1; j < m; ++j) sum = sum + crust_term(vs, zd, j);
            } else {
                double r0 = crust_term(vs, zd, 0), r1 = crust_term(vs, zd, 1), r2 = crust_term(vs, zd, 2), r3 = crust_term(vs, zd, 3);
                double r4 = crust_term(vs, zd, 4), r5 = crust_term(vs, zd, 5), r6 = crust_term(vs, zd, 6), r7 = crust_term(vs, zd, 7);
                int i = 8;
                for (; i + 8 <= m; i += 8) {
                    r0 = r0 + crust_term(vs, zd, i);
                    r1 = r1 + crust_term(vs, zd, i + 1);
                    r2 = r2 + crust_term(vs, zd, i + 2);
                    r3 = r3 + crust_term(vs, zd, i + 3);
                    r4 = r4 + crust_term(vs, zd, i + 4);
                    r5 = r5 + crust_term(vs, zd, i + 5);
                    r6 = r6 + crust_term(vs, zd, i + 6);
                    r7 = r7 + crust_term(vs, zd, i + 7);
                }
                sum = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
                for (; i < m; ++i) sum = sum + crust_term(vs, zd, i);
            }
            moho = d[k];
            last = (double)vs[k];
            crust = sum / moho;
            jump = (double)(T)(vs[k + 1] - vs[k]);
        }
        val[r] = moho;
        val[nrows + r] = last;
        val[2 * nrows + r] = crust;
        val[3 * nrows + r] = jump;
    }
    agg_add(found, s, r < nrows && k >= 0);
}

// one lane per loaded row: its value row, by its index in the loaded input; column Q = nlayers where asked
template <typename T>
__global__ void __launch_bounds__(256) sc_attach_kernel(int64_t nrows, const int64_t *porig, const int32_t *pn, int Q,
                                                        int64_t ld, const T *values, int with_nl, double *val)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    const T *v = values + porig[r] * ld;
    for (int q = 0; q < Q; ++q) val[(int64_t)q * nrows + r] = (double)v[q];
    if (with_nl) val[(int64_t)Q * nrows + r] = (double)(pn[r] - 1);
}

__global__ void __launch_bounds__(SC_THREADS) sc_stats_kernel(SetArgs a, unsigned long long *count, unsigned long long *nnan,
                                                              unsigned long long *kmin, unsigned long long *kmax, int *low,
                                                              int *not_f32)
{
    const PostWork w = a.work[blockIdx.x];
    const int q = blockIdx.y;
    const double *col = a.val + (int64_t)q * a.nrows;
    unsigned long long cnt = 0, nn = 0, mn = ~0ull, mx = 0;
    int lo = INT_MAX, nf = 0;
    for (int64_t r = w.r0 + threadIdx.x; r < w.r1; r += SC_THREADS) {
        const double v = col[r];
        if (v != v) { ++nn; continue; }
        ++cnt;
        const unsigned long long k = okey(v, false);
        mn = k < mn ? k : mn;
        mx = k > mx ? k : mx;
        const int b = low_bit(v);
        lo = b < lo ? b : lo;
        nf |= ((double)(float)v == v) ? 0 : 1;
    }
    cnt = wave_sum(cnt);
    nn = wave_sum(nn);
    mn = wave_min(mn);
    mx = wave_max(mx);
    lo = wave_min_i(lo);
    const bool anynf = __ballot(nf != 0) != 0ull;
    if (__lane_id() != 0) return;
    const size_t c = (size_t)w.site * a.Q + q;
    if (cnt) {
        atomicAdd(&count[c], cnt);
        atomicMin(&kmin[c], mn);
        atomicMax(&kmax[c], mx);
        atomicMin(&low[c], lo);
    }
    if (nn) atomicAdd(&nnan[c], nn);
    if (anynf) atomicOr(&not_f32[q], 1);
}

__global__ void __launch_bounds__(SC_THREADS) sc_moments_kernel(SetArgs a, const int32_t *scale, const int64_t *x0,
                                                                unsigned long long *sums)
{
    const PostWork w = a.work[blockIdx.x];
    const int q = blockIdx.y;
    const size_t c = (size_t)w.site * a.Q + q;
    const double *col = a.val + (int64_t)q * a.nrows;
    const int L = scale[c];
    const long long X0 = (long long)x0[c];
    const unsigned long long M = 0xffffffffull;
    unsigned long long s[6] = {0, 0, 0, 0, 0, 0};
    for (int64_t r = w.r0 + threadIdx.x; r < w.r1; r += SC_THREADS) {
        const double v = col[r];
        if (v != v) continue;
        const long long X = (long long)rint(ldexp(v, -L)); // |X| < 2^62 by the choice of L (an integer where it is exact)
        const unsigned long long Y = (unsigned long long)(X - X0);
        s[0] += Y & M;
        s[1] += Y >> 32;
        const unsigned long long lo = Y * Y, hi = __umul64hi(Y, Y);
        s[2] += lo & M;
        s[3] += lo >> 32;
        s[4] += hi & M;
        s[5] += hi >> 32;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) s[i] = wave_sum(s[i]);
    if (__lane_id() != 0) return;
    unsigned long long *o = sums + c * 6;
#pragma unroll
    for (int i = 0; i < 6; ++i)
        if (s[i]) atomicAdd(&o[i], s[i]);
}

struct EdgeArgs {
    const int64_t *off; // [S+1]
    const double *edges;
};

__global__ void __launch_bounds__(SC_THREADS) sc_hist_kernel(SetArgs a, int col, EdgeArgs e, const int64_t *cnt_off,
                                                             unsigned *counts)
{
    __shared__ unsigned h[SC_LDS_BINS];
    __shared__ double eds[SC_LDS_BINS + 1];
    const PostWork w = a.work[blockIdx.x];
    const int s = w.site;
    const int nb = (int)(e.off[s + 1] - e.off[s]) - 1;
    const double *eg = e.edges + e.off[s];
    unsigned *out = counts + cnt_off[s];
    const bool lds = nb <= SC_LDS_BINS; // (uniform over the workgroup)
    if (lds) {
        for (int b = threadIdx.x; b <= nb; b += SC_THREADS) eds[b] = eg[b];
        for (int b = threadIdx.x; b < nb; b += SC_THREADS) h[b] = 0u;
        __syncthreads();
    }
    const double *ed = lds ? eds : eg;
    const double *v = a.val + (int64_t)col * a.nrows;
    for (int64_t r = w.r0 + threadIdx.x; r < w.r1; r += SC_THREADS) {
        const double x = v[r];
        if (x != x) continue;
        const int b = find_bin(ed, nb, x);
        if (b < 0 || b >= nb) continue;
        if (lds) atomicAdd(&h[b], 1u);
        else atomicAdd(&out[b], 1u);
    }
    if (!lds) return;
    __syncthreads();
    for (int b = threadIdx.x; b < nb; b += SC_THREADS)
        if (h[b]) atomicAdd(&out[b], h[b]);
}

__global__ void __launch_bounds__(SC_THREADS) sc_hist2d_kernel(SetArgs a, int colx, int coly, EdgeArgs ex, EdgeArgs ey,
                                                               const int64_t *cnt_off, unsigned *counts)
{
    __shared__ unsigned h[SC_LDS_CELLS];
    __shared__ double eds[SC_LDS_EDGES];
    const PostWork w = a.work[blockIdx.x];
    const int s = w.site;
    const int nx = (int)(ex.off[s + 1] - ex.off[s]) - 1, ny = (int)(ey.off[s + 1] - ey.off[s]) - 1;
    const double *gx = ex.edges + ex.off[s], *gy = ey.edges + ey.off[s];
    unsigned *out = counts + cnt_off[s];
    const int64_t cells = (int64_t)nx * ny;
    const bool lds = cells <= SC_LDS_CELLS && nx + ny + 2 <= SC_LDS_EDGES; // (uniform over the workgroup)
    if (lds) {
        for (int b = threadIdx.x; b <= nx; b += SC_THREADS) eds[b] = gx[b];
        for (int b = threadIdx.x; b <= ny; b += SC_THREADS) eds[nx + 1 + b] = gy[b];
        for (int b = threadIdx.x; b < (int)cells; b += SC_THREADS) h[b] = 0u;
        __syncthreads();
    }
    const double *edx = lds ? eds : gx, *edy = lds ? eds + nx + 1 : gy;
    const double *vx = a.val + (int64_t)colx * a.nrows, *vy = a.val + (int64_t)coly * a.nrows;
    for (int64_t r = w.r0 + threadIdx.x; r < w.r1; r += SC_THREADS) {
        const double x = vx[r], y = vy[r];
        if (x != x || y != y) continue;
        const int bx = find_bin(edx, nx, x), by = find_bin(edy, ny, y);
        if (bx < 0 || bx >= nx || by < 0 || by >= ny) continue;
        const int64_t cell = (int64_t)bx * ny + by;
        if (lds) atomicAdd(&h[cell], 1u);
        else atomicAdd(&out[cell], 1u);
    }
    if (!lds) return;
    __syncthreads();
    for (int b = threadIdx.x; b < (int)cells; b += SC_THREADS)
        if (h[b]) atomicAdd(&out[b], h[b]);
}

// one workgroup per site: the first largest cell of its flattened counts
__global__ void __launch_bounds__(256) sc_argmax_kernel(const int64_t *cnt_off, const int64_t *ncell, const unsigned *counts,
                                                        long long *argmax)
{
    __shared__ unsigned bv[256];
    __shared__ long long bi[256];
    const int s = blockIdx.x;
    const unsigned *c = counts + cnt_off[s];
    const int64_t n = ncell[s];
    unsigned v = 0;
    long long idx = LLONG_MAX;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const unsigned x = c[i];
        if (idx == LLONG_MAX || x > v) { v = x; idx = i; } // (ascending i: the first of equal counts stays)
    }
    bv[threadIdx.x] = v;
    bi[threadIdx.x] = idx;
    __syncthreads();
    for (int o = 128; o; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const unsigned v2 = bv[threadIdx.x + o];
            const long long i2 = bi[threadIdx.x + o];
            const long long i1 = bi[threadIdx.x];
            if (i2 != LLONG_MAX && (i1 == LLONG_MAX || v2 > bv[threadIdx.x] || (v2 == bv[threadIdx.x] && i2 < i1))) {
                bv[threadIdx.x] = v2;
                bi[threadIdx.x] = i2;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) argmax[s] = bi[0] == LLONG_MAX ? -1 : bi[0];
}

// ---- host side ---------------------------------------------------------------------------------------------------

// per-site edges: offsets from 0, at least 2 finite ascending edges each; nb[s] = the bins
int check_edges(bh_posterior *p, const int64_t *off, const double *edges, std::vector<int64_t> &nb)
{
    if (!off || !edges) return pfail(p, BH_EINVAL, "null argument");
    if (off[0] != 0) return pfail(p, BH_EINVAL, "edge offsets must start at 0");
    nb.resize(p->S);
    for (int s = 0; s < p->S; ++s) {
        nb[s] = off[s + 1] - off[s] - 1;
        if (nb[s] < 1 || nb[s] > (int64_t)BH_POSTERIOR_MAXCOUNTS)
            return pfail(p, BH_EINVAL, "every site needs 2 .. BH_POSTERIOR_MAXCOUNTS + 1 edges");
        for (int64_t i = off[s]; i <= off[s] + nb[s]; ++i)
            if (!std::isfinite(edges[i]) || (i > off[s] && edges[i] < edges[i - 1]))
                return pfail(p, BH_EINVAL, "edges must be finite and ascending");
    }
    return BH_OK;
}

int upload_edges(bh_posterior *p, Dev &doff, Dev &ded, const int64_t *off, const double *edges)
{
    int rc;
    const size_t ne = (size_t)off[p->S];
    if ((rc = alloc(p, doff, (size_t)(p->S + 1) * 8)) || (rc = alloc(p, ded, ne * 8))) return rc;
    PCHK(p, hipMemcpyAsync(doff.p, off, (size_t)(p->S + 1) * 8, hipMemcpyHostToDevice, p->st));
    PCHK(p, hipMemcpyAsync(ded.p, edges, ne * 8, hipMemcpyHostToDevice, p->st));
    return BH_OK;
}

} // namespace

extern "C" {

int bh_posterior_keep_rows(bh_posterior *p, int on)
{
    if (!p) return BH_EINVAL;
    p->keep_rows = on != 0;
    return BH_OK;
}

int bh_posterior_moho(bh_posterior *p, const double *lo, const double *hi, const double *mohovs, int64_t *found)
{
    int rc;
    if (!p) return BH_EINVAL;
    if (p->S < 1) return pfail(p, BH_EINVAL, "no rows loaded (bh_posterior_load)");
    if (!p->has_rows) return pfail(p, BH_EINVAL, "the rows were loaded without bh_posterior_keep_rows");
    if (!lo || !hi || !mohovs) return pfail(p, BH_EINVAL, "null argument");
    const int S = p->S;
    for (int s = 0; s < S; ++s) {
        if (!std::isfinite(lo[s]) || !std::isfinite(hi[s]) || !std::isfinite(mohovs[s]))
            return pfail(p, BH_EINVAL, "the Moho range and mohovs must be finite");
        if (lo[s] < 0.0) return pfail(p, BH_EINVAL, "the Moho range must not start below 0 km");
        if (!(hi[s] > lo[s])) return pfail(p, BH_EINVAL, "the Moho range needs lo < hi");
    }
    PCHK(p, hipSetDevice(p->device));
    ScalarSet &ss = p->sets[BH_SCALARS_MOHO];
    ss.drop();
    const size_t nr = (size_t)p->nrows;
    Dev dpar, dfound;
    if ((rc = alloc(p, ss.val, nr * 4 * 8)) || (rc = alloc(p, dpar, (size_t)S * 3 * 8)) || (rc = alloc(p, dfound, (size_t)S * 8)))
        return rc;
    double *par = dpar.as<double>();
    PCHK(p, hipMemcpyAsync(par, lo, (size_t)S * 8, hipMemcpyHostToDevice, p->st));
    PCHK(p, hipMemcpyAsync(par + S, hi, (size_t)S * 8, hipMemcpyHostToDevice, p->st));
    PCHK(p, hipMemcpyAsync(par + 2 * S, mohovs, (size_t)S * 8, hipMemcpyHostToDevice, p->st));
    PCHK(p, hipMemsetAsync(dfound.p, 0, (size_t)S * 8, p->st));
    if (nr) {
        const unsigned nblk = (unsigned)((nr + 255) / 256);
        if (p->elem == 4)
            sc_moho_kernel<float><<<nblk, 256, 0, p->st>>>(p->nrows, p->ML, p->pn.as<int32_t>(), p->psite.as<int32_t>(), p->pvs.as<float>(),
                p->pzd.as<float>(), p->pd.as<double>(), par, par + S, par + 2 * S, ss.val.as<double>(), dfound.as<unsigned long long>());
        else
            sc_moho_kernel<double><<<nblk, 256, 0, p->st>>>(p->nrows, p->ML, p->pn.as<int32_t>(), p->psite.as<int32_t>(), p->pvs.as<double>(),
                p->pzd.as<double>(), p->pd.as<double>(), par, par + S, par + 2 * S, ss.val.as<double>(), dfound.as<unsigned long long>());
        PCHK(p, hipGetLastError());
    }
    std::vector<unsigned long long> hf(S);
    PCHK(p, hipMemcpyAsync(hf.data(), dfound.p, (size_t)S * 8, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipStreamSynchronize(p->st));
    if (found)
        for (int s = 0; s < S; ++s) found[s] = (int64_t)hf[s];
    ss.Q = 4;
    return BH_OK;
}

int bh_posterior_attach(bh_posterior *p, int memspace, void *stream, int elem_bytes, int Q, int64_t ld, const void *values,
                        int with_nlayers)
{
    int rc;
    if (!p) return BH_EINVAL;
    if (p->S < 1) return pfail(p, BH_EINVAL, "no rows loaded (bh_posterior_load)");
    if (!p->has_rows) return pfail(p, BH_EINVAL, "the rows were loaded without bh_posterior_keep_rows");
    if (elem_bytes != 4 && elem_bytes != 8) return pfail(p, BH_EINVAL, "values must be float32 or float64");
    if (Q < 0 || Q > BH_SCALARS_MAXCOLS) return pfail(p, BH_EINVAL, "columns: 0..BH_SCALARS_MAXCOLS");
    if (Q == 0 && !with_nlayers) return pfail(p, BH_EINVAL, "no column to attach");
    if (Q && (ld < Q || (!values && p->ninput))) return pfail(p, BH_EINVAL, "bad row stride or null values");
    PCHK(p, hipSetDevice(p->device));
    const bool host = memspace != BH_DEVICE;
    p->st = (!host && stream) ? (hipStream_t)stream : (hipStream_t)bh_engine_stream(p->e);
    ScalarSet &ss = p->sets[BH_SCALARS_USER];
    ss.drop();
    const int ncols = Q + (with_nlayers ? 1 : 0);
    const size_t nr = (size_t)p->nrows, eb = (size_t)elem_bytes;
    Dev dv;
    const void *v = values;
    if (host && Q && p->ninput) {
        const size_t n = (size_t)((p->ninput - 1) * ld + Q);
        if ((rc = alloc(p, dv, n * eb))) return rc;
        PCHK(p, hipMemcpyAsync(dv.p, values, n * eb, hipMemcpyHostToDevice, p->st));
        v = dv.p;
    }
    if ((rc = alloc(p, ss.val, nr * ncols * 8))) return rc;
    if (nr) {
        const unsigned nblk = (unsigned)((nr + 255) / 256);
        if (elem_bytes == 4)
            sc_attach_kernel<float><<<nblk, 256, 0, p->st>>>(p->nrows, p->porig.as<int64_t>(), p->pn.as<int32_t>(), Q, ld, (const float *)v,
                                                             with_nlayers ? 1 : 0, ss.val.as<double>());
        else
            sc_attach_kernel<double><<<nblk, 256, 0, p->st>>>(p->nrows, p->porig.as<int64_t>(), p->pn.as<int32_t>(), Q, ld, (const double *)v,
                                                              with_nlayers ? 1 : 0, ss.val.as<double>());
        PCHK(p, hipGetLastError());
    }
    PCHK(p, hipStreamSynchronize(p->st));
    ss.Q = ncols;
    return BH_OK;
}

int bh_posterior_scalar_cols(bh_posterior *p, int set, int32_t *ncols)
{
    int rc;
    if (!p) return BH_EINVAL;
    ScalarSet *ss;
    if ((rc = get_set(p, set, &ss))) return rc;
    if (!ncols) return pfail(p, BH_EINVAL, "null argument");
    *ncols = ss->Q;
    return BH_OK;
}

int bh_posterior_scalar_stats(bh_posterior *p, int set, int64_t *count, int64_t *nnan, uint64_t *kmin, uint64_t *kmax,
                              int32_t *scale, int64_t *x0, int32_t *exact, uint64_t *sums, uint64_t *median)
{
    int rc;
    if (!p) return BH_EINVAL;
    ScalarSet *ss;
    if ((rc = get_set(p, set, &ss))) return rc;
    if (!count || !nnan || !kmin || !kmax || !scale || !x0 || !exact || !sums) return pfail(p, BH_EINVAL, "null argument");
    PCHK(p, hipSetDevice(p->device));
    const int Q = ss->Q;
    const size_t ncol = (size_t)p->S * Q;
    Dev dcnt, dnan, dmin, dmax, dlow, dnf, dsc, dx0, dsum;
    if ((rc = alloc(p, dcnt, ncol * 8)) || (rc = alloc(p, dnan, ncol * 8)) || (rc = alloc(p, dmin, ncol * 8)) ||
        (rc = alloc(p, dmax, ncol * 8)) || (rc = alloc(p, dlow, ncol * 4)) || (rc = alloc(p, dnf, (size_t)Q * 4)))
        return rc;
    PCHK(p, hipMemsetAsync(dcnt.p, 0, ncol * 8, p->st));
    PCHK(p, hipMemsetAsync(dnan.p, 0, ncol * 8, p->st));
    PCHK(p, hipMemsetAsync(dmin.p, 0xff, ncol * 8, p->st));
    PCHK(p, hipMemsetAsync(dmax.p, 0, ncol * 8, p->st));
    PCHK(p, hipMemsetAsync(dlow.p, 0x7f, ncol * 4, p->st)); // 0x7f7f7f7f: above every exponent
    PCHK(p, hipMemsetAsync(dnf.p, 0, (size_t)Q * 4, p->st));
    const SetArgs a = set_args(p, ss);
    const dim3 grid((unsigned)p->work.size(), (unsigned)Q);
    if (!p->work.empty()) {
        sc_stats_kernel<<<grid, SC_THREADS, 0, p->st>>>(a, dcnt.as<unsigned long long>(), dnan.as<unsigned long long>(),
                                                        dmin.as<unsigned long long>(), dmax.as<unsigned long long>(), dlow.as<int>(),
                                                        dnf.as<int>());
        PCHK(p, hipGetLastError());
    }
    std::vector<int32_t> low(ncol), nf(Q);
    PCHK(p, hipMemcpyAsync(count, dcnt.p, ncol * 8, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipMemcpyAsync(nnan, dnan.p, ncol * 8, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipMemcpyAsync(kmin, dmin.p, ncol * 8, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipMemcpyAsync(kmax, dmax.p, ncol * 8, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipMemcpyAsync(low.data(), dlow.p, ncol * 4, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipMemcpyAsync(nf.data(), dnf.p, (size_t)Q * 4, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipStreamSynchronize(p->st));
    ss->count.assign(count, count + ncol);   // (for bh_posterior_scalar_quantiles)
    ss->nf.assign(nf.begin(), nf.end());
    for (size_t c = 0; c < ncol; ++c) {   // the fixed-point scale of every column
        if (count[c] == 0) { scale[c] = 0; x0[c] = 0; exact[c] = 1; continue; }
        if ((rc = scale_rule(p, kmin[c], kmax[c], low[c], "a value of a scalar column is not finite", &scale[c], &x0[c], &exact[c])))
            return rc;
    }
    if ((rc = alloc(p, dsc, ncol * 4)) || (rc = alloc(p, dx0, ncol * 8)) || (rc = alloc(p, dsum, ncol * 48))) return rc;
    PCHK(p, hipMemcpyAsync(dsc.p, scale, ncol * 4, hipMemcpyHostToDevice, p->st));
    PCHK(p, hipMemcpyAsync(dx0.p, x0, ncol * 8, hipMemcpyHostToDevice, p->st));
    PCHK(p, hipMemsetAsync(dsum.p, 0, ncol * 48, p->st));
    if (!p->work.empty()) {
        sc_moments_kernel<<<grid, SC_THREADS, 0, p->st>>>(a, dsc.as<int32_t>(), dx0.as<int64_t>(), dsum.as<unsigned long long>());
        PCHK(p, hipGetLastError());
    }
    PCHK(p, hipMemcpyAsync(sums, dsum.p, ncol * 48, hipMemcpyDeviceToHost, p->st));
    if (median) {   // the keys of ranks (n-1)/2 and (n-1)/2 + 1; a column of float32-exact values is selected on 32-bit keys
        std::vector<uint32_t> rk(ncol);
        std::vector<int> kb(Q);
        for (int q = 0; q < Q; ++q) kb[q] = nf[q] ? 64 : 32;
        for (size_t c = 0; c < ncol; ++c) rk[c] = count[c] ? (uint32_t)((count[c] - 1) / 2) : 0u;
        if ((rc = select_ranks(p, ncol, 1, rk.data(), count, kb, true, SetSelect{p, a}, median, median + 1, 2))) return rc;
    }
    PCHK(p, hipStreamSynchronize(p->st));
    return BH_OK;
}

int bh_posterior_scalar_hist(bh_posterior *p, int set, int col, const int64_t *edge_off, const double *edges, uint32_t *counts)
{
    int rc;
    if (!p) return BH_EINVAL;
    ScalarSet *ss;
    if ((rc = get_set(p, set, &ss))) return rc;
    if (col < 0 || col >= ss->Q) return pfail(p, BH_EINVAL, "column out of range");
    if (!counts) return pfail(p, BH_EINVAL, "null argument");
    std::vector<int64_t> nb, coff(p->S);
    if ((rc = check_edges(p, edge_off, edges, nb))) return rc;
    int64_t ncells = 0;
    for (int s = 0; s < p->S; ++s) {
        coff[s] = ncells;
        ncells += nb[s];
        if (ncells > (int64_t)BH_POSTERIOR_MAXCOUNTS) return pfail(p, BH_EINVAL, "the histogram would exceed BH_POSTERIOR_MAXCOUNTS (2^27) cells");
    }
    PCHK(p, hipSetDevice(p->device));
    Dev deo, ded, dco, dcnt;
    if ((rc = upload_edges(p, deo, ded, edge_off, edges))) return rc;
    if ((rc = alloc(p, dco, (size_t)p->S * 8)) || (rc = alloc(p, dcnt, (size_t)ncells * 4))) return rc;
    PCHK(p, hipMemcpyAsync(dco.p, coff.data(), (size_t)p->S * 8, hipMemcpyHostToDevice, p->st));
    PCHK(p, hipMemsetAsync(dcnt.p, 0, (size_t)ncells * 4, p->st));
    if (!p->work.empty()) {
        const EdgeArgs e{deo.as<int64_t>(), ded.as<double>()};
        sc_hist_kernel<<<(unsigned)p->work.size(), SC_THREADS, 0, p->st>>>(set_args(p, ss), col, e, dco.as<int64_t>(), dcnt.as<unsigned>());
        PCHK(p, hipGetLastError());
    }
    PCHK(p, hipMemcpyAsync(counts, dcnt.p, (size_t)ncells * 4, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipStreamSynchronize(p->st));
    return BH_OK;
}

int bh_posterior_scalar_hist2d(bh_posterior *p, int set, int colx, int coly, const int64_t *xedge_off, const double *xedges,
                               const int64_t *yedge_off, const double *yedges, uint32_t *counts, int64_t *argmax)
{
    int rc;
    if (!p) return BH_EINVAL;
    ScalarSet *ss;
    if ((rc = get_set(p, set, &ss))) return rc;
    if (colx < 0 || colx >= ss->Q || coly < 0 || coly >= ss->Q) return pfail(p, BH_EINVAL, "column out of range");
    if (!counts) return pfail(p, BH_EINVAL, "null argument");
    const int S = p->S;
    std::vector<int64_t> nx, ny, coff(S), ncell(S);
    if ((rc = check_edges(p, xedge_off, xedges, nx)) || (rc = check_edges(p, yedge_off, yedges, ny))) return rc;
    int64_t ncells = 0;
    for (int s = 0; s < S; ++s) {
        coff[s] = ncells;
        if (nx[s] > (int64_t)BH_POSTERIOR_MAXCOUNTS / ny[s] || ncells + nx[s] * ny[s] > (int64_t)BH_POSTERIOR_MAXCOUNTS)
            return pfail(p, BH_EINVAL, "the histogram would exceed BH_POSTERIOR_MAXCOUNTS (2^27) cells");
        ncell[s] = nx[s] * ny[s];
        ncells += ncell[s];
    }
    PCHK(p, hipSetDevice(p->device));
    Dev dxo, dxe, dyo, dye, dco, dnc, dcnt, dam;
    if ((rc = upload_edges(p, dxo, dxe, xedge_off, xedges)) || (rc = upload_edges(p, dyo, dye, yedge_off, yedges))) return rc;
    if ((rc = alloc(p, dco, (size_t)S * 8)) || (rc = alloc(p, dnc, (size_t)S * 8)) || (rc = alloc(p, dcnt, (size_t)ncells * 4))) return rc;
    PCHK(p, hipMemcpyAsync(dco.p, coff.data(), (size_t)S * 8, hipMemcpyHostToDevice, p->st));
    PCHK(p, hipMemcpyAsync(dnc.p, ncell.data(), (size_t)S * 8, hipMemcpyHostToDevice, p->st));
    PCHK(p, hipMemsetAsync(dcnt.p, 0, (size_t)ncells * 4, p->st));
    if (!p->work.empty()) {
        const EdgeArgs ex{dxo.as<int64_t>(), dxe.as<double>()}, ey{dyo.as<int64_t>(), dye.as<double>()};
        sc_hist2d_kernel<<<(unsigned)p->work.size(), SC_THREADS, 0, p->st>>>(set_args(p, ss), colx, coly, ex, ey, dco.as<int64_t>(),
                                                                             dcnt.as<unsigned>());
        PCHK(p, hipGetLastError());
    }
    if (argmax) {
        if ((rc = alloc(p, dam, (size_t)S * 8))) return rc;
        sc_argmax_kernel<<<(unsigned)S, 256, 0, p->st>>>(dco.as<int64_t>(), dnc.as<int64_t>(), dcnt.as<unsigned>(), dam.as<long long>());
        PCHK(p, hipGetLastError());
        PCHK(p, hipMemcpyAsync(argmax, dam.p, (size_t)S * 8, hipMemcpyDeviceToHost, p->st));
    }
    PCHK(p, hipMemcpyAsync(counts, dcnt.p, (size_t)ncells * 4, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipStreamSynchronize(p->st));
    return BH_OK;
}

} // extern "C"
