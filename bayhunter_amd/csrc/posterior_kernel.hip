// bayhunter_amd/csrc/posterior_kernel.hip -- posterior velocity-depth summaries of many sites (include/bh_engine_posterior.h).
//
// Load: one lane per row validates it, forms its interface depths and scatters it to its site's slice (a counting sort:
// per-site counts, host prefix sum, a cursor per site).  Inside a slice the order of rows is not fixed -- nothing below
// depends on it: every result is a count, a min / max, an integer sum or a selection, all independent of the order.
//
// Column passes: a workgroup is one wavefront = 64 depths of one site over a chunk of at most CHUNK rows of it.  Every
// lane reads the same row (uniform, scalar loads) and takes vs[#{d_j <= x}] for its depth x.  Chunk results meet in
// integer atomics (min / max of ordered keys, counts, 64-bit limb sums), so the results are the same bits in every run.
//   stats   : min, max and the lowest set bit of every column (for the fixed-point scale of the sums)
//   moments : the 32-bit limbs of sum(Y) and sum(Y^2), Y = v * 2^-scale - X0 an integer (exact where scale allows)
//   radix   : the median and the quantiles by the radix select of posterior_select.h on the ordered key, 8 bits per pass (4
//             passes for float32 keys, 8 for float64); per-lane 256-bin histograms in LDS as pairs of 16-bit counters (CHUNK <
//             2^16).  A last pass finds the next key above the selected one (the upper middle of an even count).
//   hist    : counts over the caller's vs edges (binary search, 'right', last edge to the last bin) and depth bins;
//             in LDS when every site has at most 256 vs bins, else straight to global atomics.
// -ffp-contract=off (Makefile) keeps (z_j + z_{j+1}) / 2 and the cumulative sums rounded as numpy rounds them.
#include "posterior_select.h"
#include "../../include/bh_engine_posterior_quantiles.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#define POST_HIST_LDS_BINS 256
#define POST_IFACE_LDS_BINS 4096

using namespace bhpost;

namespace {

// n >= 1 layers, 0 = NaN only, -1 = the non-NaN values are not a prefix of even length
template <typename T>
__device__ int row_layers(const T *row, int W)
{
    int c = 0, first = W;
    for (int i = 0; i < W; ++i) {
        const bool nan = row[i] != row[i];
        c += nan ? 0 : 1;
        first = (nan && i < first) ? i : first;
    }
    if (c == 0) return 0;
    if (c != first || (c & 1)) return -1;
    return c / 2;
}

template <typename T>
__global__ void __launch_bounds__(256) post_count_kernel(int64_t N, int W, int64_t ld, const T *models, const int32_t *site,
                                                         int S, unsigned long long *rows, unsigned long long *invalid,
                                                         unsigned long long *dropped, int *not_f32)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int s = -1, n = 0;
    if (r < N) {
        s = site ? site[r] : 0;
        if (s < 0 || s >= S) {
            atomicAdd(dropped, 1ull);
            s = -1;
        } else {
            const T *row = models + r * ld;
            n = row_layers(row, W);
            if (n < 0) atomicAdd(&invalid[s], 1ull);
            if (sizeof(T) == 8 && n > 0) {
                bool f = true;
                for (int j = 0; j < n; ++j) f = f && ((double)(float)row[j] == (double)row[j]);
                if (!f) atomicOr(not_f32, 1);
            }
        }
    }
    agg_add(rows, s < 0 ? 0 : s, s >= 0 && n > 0);
}

// the kept rows to their site's slice: n, vs (row dtype), d (float64: the step model's depths), di (float32 rows: the
// interface depths in float32, _replace_zvnoi_h; float64 rows use d); for the scalar sets (posterior_scalars_kernel.hip) the
// row's index in the input and its zd_j in the row's dtype, where the handle asks for them (bh_posterior_keep_rows)
template <typename T>
__global__ void __launch_bounds__(256) post_scatter_kernel(int64_t N, int W, int64_t ld, const T *models, const int32_t *site,
                                                           int S, int ML, unsigned long long *cursor, int32_t *pn,
                                                           int32_t *psite, T *pvs, double *pd, float *pdi, int64_t *porig, T *pzd)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int s = -1, n = 0;
    const T *row = models + (r < N ? r : 0) * ld;
    if (r < N) {
        s = site ? site[r] : 0;
        if (s >= 0 && s < S) n = row_layers(row, W);
        else s = -1;
    }
    const bool on = s >= 0 && n > 0;
    const unsigned long long pos = agg_add(cursor, on ? s : 0, on);
    if (!on) return;
    pn[pos] = n;
    psite[pos] = s;
    if (porig) porig[pos] = r;   // (bh_posterior_keep_rows)
    T *vs = pvs + pos * ML;
    double *d = pd + pos * ML;
    for (int j = 0; j < n; ++j) vs[j] = row[j];
    const T *z = row + n;
    T zprev = (T)0;
    double dsum = 0.0;
    float isum = 0.0f;
    for (int j = 0; j < n - 1; ++j) {
        const T zd = (z[j] + z[j + 1]) / (T)2;
        const double h = (double)zd - (double)zprev; // numpy: z_disc - concatenate(([0], z_disc[:-1])) is float64
        dsum = j ? dsum + h : h;
        d[j] = dsum;
        if (pzd) pzd[pos * ML + j] = zd;
        if (pdi) {
            const float hf = (float)h;               // written back into the float32 model row
            isum = j ? isum + hf : hf;
            pdi[pos * ML + j] = isum;
        }
        zprev = zd;
    }
}

// vs of a row at depth x: vs[#{j : d_j <= x}]
template <typename T>
__device__ __forceinline__ double sample(int n, const T *vs, const double *d, double x)
{
    int k = 0;
    for (int j = 0; j < n - 1; ++j) k += d[j] <= x ? 1 : 0;
    double v = (double)vs[0];
    for (int j = 1; j < n; ++j) v = k == j ? (double)vs[j] : v;
    return v;
}

struct ColArgs {
    const PostWork *work;
    const int32_t *pn;
    const void *pvs;
    const double *pd;
    int ML, D;
    const double *dep;
};

template <typename T>
__global__ void __launch_bounds__(64) post_stats_kernel(ColArgs a, unsigned long long *kmin, unsigned long long *kmax, int *low)
{
    const PostWork w = a.work[blockIdx.x];
    const int j = blockIdx.y * 64 + threadIdx.x;
    const bool act = j < a.D;
    const double x = act ? a.dep[j] : 0.0;
    const T *pvs = (const T *)a.pvs;
    unsigned long long mn = ~0ull, mx = 0;
    int lo = INT_MAX;
    for (int64_t r = w.r0; r < w.r1; ++r) {
        const double v = sample(a.pn[r], pvs + r * a.ML, a.pd + r * a.ML, x);
        const unsigned long long k = okey(v, false);
        mn = k < mn ? k : mn;
        mx = k > mx ? k : mx;
        const int b = low_bit(v);
        lo = b < lo ? b : lo;
    }
    if (!act) return;
    const size_t c = (size_t)w.site * a.D + j;
    atomicMin(&kmin[c], mn);
    atomicMax(&kmax[c], mx);
    atomicMin(&low[c], lo);
}

template <typename T>
__global__ void __launch_bounds__(64) post_moments_kernel(ColArgs a, const int32_t *scale, const int64_t *x0, unsigned long long *sums)
{
    const PostWork w = a.work[blockIdx.x];
    const int j = blockIdx.y * 64 + threadIdx.x;
    const bool act = j < a.D;
    const size_t c = (size_t)w.site * a.D + (act ? j : 0);
    const double x = act ? a.dep[j] : 0.0;
    const int L = act ? scale[c] : 0;
    const long long X0 = act ? (long long)x0[c] : 0;
    const T *pvs = (const T *)a.pvs;
    const unsigned long long M = 0xffffffffull;
    unsigned long long s0 = 0, s1 = 0, q0 = 0, q1 = 0, q2 = 0, q3 = 0;
    for (int64_t r = w.r0; r < w.r1; ++r) {
        const double v = sample(a.pn[r], pvs + r * a.ML, a.pd + r * a.ML, x);
        const long long X = (long long)rint(ldexp(v, -L)); // |X| < 2^62 by the choice of L (an integer where it is exact)
        const unsigned long long Y = (unsigned long long)(X - X0);
        s0 += Y & M;
        s1 += Y >> 32;
        const unsigned long long lo = Y * Y, hi = __umul64hi(Y, Y);
        q0 += lo & M;
        q1 += lo >> 32;
        q2 += hi & M;
        q3 += hi >> 32;
    }
    if (!act) return;
    unsigned long long *o = sums + c * 6;
    atomicAdd(&o[0], s0);
    atomicAdd(&o[1], s1);
    atomicAdd(&o[2], q0);
    atomicAdd(&o[3], q1);
    atomicAdd(&o[4], q2);
    atomicAdd(&o[5], q3);
}

// ---- the order statistics of a column (posterior_select.h): the column layout's radix and next pass -------------------------

// the radix pass of ONE rank, written out, and the only radix pass ColSelect launches for NR = 1: col_radix_kernel<T, 1> is never
// instantiated.  It has the same registers, LDS and occupancy and 12 instructions fewer, but put a posterior_models call of 64
// sites x 200 000 rows 0.7 % above the spread of the parent's repeats (profiles/posterior_select_refactor.txt, sections 2 and
// 3).  A copy kept on a difference this small: to re-test, launch col_radix_kernel<T, 1> from ColSelect::radix, run
// tools/gpu_posterior_perf.py alternately on both builds, and delete this kernel if the two lie within each other's spread.
template <typename T>
__global__ void __launch_bounds__(64) col_radix1_kernel(ColArgs a, int k32, int shift, const unsigned long long *pref,
                                                        unsigned *ghist)
{
    __shared__ unsigned h[128 * 64]; // [digit / 2][lane]: two 16-bit counters
    const PostWork w = a.work[blockIdx.x];
    const int lane = threadIdx.x;
    const int j = blockIdx.y * 64 + lane;
    const bool act = j < a.D;
    for (int b = 0; b < 128; ++b) h[b * 64 + lane] = 0u; // a lane touches its own column only: no barrier
    if (!act) return;
    const size_t c = (size_t)w.site * a.D + j;
    const double x = a.dep[j];
    const unsigned long long p = pref[c];
    const int hs = shift + 8;
    const T *pvs = (const T *)a.pvs;
    for (int64_t r = w.r0; r < w.r1; ++r) {
        const double v = sample(a.pn[r], pvs + r * a.ML, a.pd + r * a.ML, x);
        const unsigned long long k = okey(v, k32 != 0);
        if (hs < 64 && ((k ^ p) >> hs) != 0ull) continue;
        const unsigned dg = (unsigned)(k >> shift) & 255u;
        h[(dg >> 1) * 64 + lane] += 1u << ((dg & 1u) * 16u);
    }
    unsigned *g = ghist + c * 256;
    for (int b = 0; b < 128; ++b) {
        const unsigned v = h[b * 64 + lane];
        if (v & 0xffffu) atomicAdd(&g[2 * b], v & 0xffffu);
        if (v >> 16) atomicAdd(&g[2 * b + 1], v >> 16);
    }
}

// one pass of the radix select: every (row, depth) is sampled once; its key is counted by its 8-bit digit at `shift` for the one
// owner whose prefix above it it matches.  Rank 0 is always an owner, and while the ranks have not parted it is the only one (a
// call of one rank takes col_radix1_kernel): its counters are the lane's private 16-bit pairs in LDS.  A rank that has left rank 0's
// prefix counts straight into its global counters.
template <typename T, int NR>
__global__ void __launch_bounds__(64) col_radix_kernel(ColArgs a, int Rarg, int k32, int shift, const unsigned long long *pref,
                                                       unsigned *ghist)
{
    __shared__ unsigned h[128 * 64]; // [digit / 2][lane]: two 16-bit counters
    const PostWork w = a.work[blockIdx.x];
    const int lane = threadIdx.x;
    const int j = blockIdx.y * 64 + lane;
    const bool act = j < a.D;
    for (int b = 0; b < 128; ++b) h[b * 64 + lane] = 0u; // a lane touches its own column only: no barrier
    if (!act) return;
    const int R = select_ranks_of<NR>(Rarg);
    const size_t c = (size_t)w.site * a.D + j;
    const double x = a.dep[j];
    const int hs = shift + 8;
    unsigned long long p[NR];
    load_prefixes<NR>(p, pref + c * R, R);
    const unsigned own = owner_mask<NR>(p, R, hs);
    const T *pvs = (const T *)a.pvs;
    unsigned *g = ghist + c * R * 256;
    for (int64_t r = w.r0; r < w.r1; ++r) {
        const double v = sample(a.pn[r], pvs + r * a.ML, a.pd + r * a.ML, x);
        const unsigned long long k = okey(v, k32 != 0);
        const unsigned dg = key_digit(k, shift);
        int o = -1;
#pragma unroll
        for (int q = 0; q < NR; ++q) o = (((own >> q) & 1u) && key_matches(k, p[q], hs)) ? q : o;
        if (o == 0) h[(dg >> 1) * 64 + lane] += 1u << ((dg & 1u) * 16u);
        else if (o > 0) atomicAdd(&g[o * 256 + dg], 1u);
    }
    for (int b = 0; b < 128; ++b) {
        const unsigned v = h[b * 64 + lane];
        if (v & 0xffffu) atomicAdd(&g[2 * b], v & 0xffffu);
        if (v >> 16) atomicAdd(&g[2 * b + 1], v >> 16);
    }
}

// per rank the number of keys <= the selected one, and the least key above it
template <typename T, int NR>
__global__ void __launch_bounds__(64) col_next_kernel(ColArgs a, int Rarg, int k32, const unsigned long long *pref, unsigned *nle,
                                                      unsigned long long *next)
{
    const PostWork w = a.work[blockIdx.x];
    const int j = blockIdx.y * 64 + threadIdx.x;
    if (j >= a.D) return;
    const int R = select_ranks_of<NR>(Rarg);
    const size_t c = (size_t)w.site * a.D + j;
    const double x = a.dep[j];
    const T *pvs = (const T *)a.pvs;
    unsigned long long p[NR], nx[NR];
    unsigned le[NR];
    load_prefixes<NR>(p, pref + c * R, R);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        le[r] = 0u;
        nx[r] = ~0ull;
    }
    for (int64_t r = w.r0; r < w.r1; ++r) {
        const unsigned long long k = okey(sample(a.pn[r], pvs + r * a.ML, a.pd + r * a.ML, x), k32 != 0);
#pragma unroll
        for (int q = 0; q < NR; ++q) {
            if (q >= R) break; // (uniform)
            le[q] += k <= p[q] ? 1u : 0u;
            nx[q] = (k > p[q] && k < nx[q]) ? k : nx[q];
        }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        if (r >= R) continue;
        atomicAdd(&nle[c * R + r], le[r]);
        atomicMin(&next[c * R + r], nx[r]);
    }
}

struct HistArgs {
    const int32_t *dbin;
    int ND;
    const int64_t *edge_off; // [S+1]
    const double *edges;
    const int64_t *cnt_off;  // [S]
    unsigned *counts;
    int lds;                 // every site has at most POST_HIST_LDS_BINS bins
};

template <typename T>
__global__ void __launch_bounds__(64) post_hist_kernel(ColArgs a, HistArgs hg)
{
    __shared__ unsigned h[(POST_HIST_LDS_BINS / 2) * 64];
    __shared__ double eds[POST_HIST_LDS_BINS + 1];
    const PostWork w = a.work[blockIdx.x];
    const int lane = threadIdx.x;
    const int j = blockIdx.y * 64 + lane;
    const int s = w.site;
    const int nb = (int)(hg.edge_off[s + 1] - hg.edge_off[s]) - 1;
    const double *eg = hg.edges + hg.edge_off[s];
    const bool act = j < a.D;
    const int db = act ? hg.dbin[j] : -1;
    unsigned *out = hg.counts + hg.cnt_off[s];
    if (hg.lds) {
        for (int b = lane; b <= nb; b += 64) eds[b] = eg[b];
        for (int b = 0; b < (nb + 1) / 2; ++b) h[b * 64 + lane] = 0u;
        __syncthreads();
    }
    if (db < 0) return; // (no barrier below)
    const double x = a.dep[j];
    const double *e = hg.lds ? eds : eg;
    const T *pvs = (const T *)a.pvs;
    for (int64_t r = w.r0; r < w.r1; ++r) {
        const double v = sample(a.pn[r], pvs + r * a.ML, a.pd + r * a.ML, x);
        const int b = find_bin(e, nb, v);
        if (b < 0 || b >= nb) continue;
        if (hg.lds) h[(b >> 1) * 64 + lane] += 1u << ((b & 1) * 16);
        else atomicAdd(&out[(size_t)b * hg.ND + db], 1u);
    }
    if (!hg.lds) return;
    for (int b = 0; b < (nb + 1) / 2; ++b) {
        const unsigned v = h[b * 64 + lane];
        if (v & 0xffffu) atomicAdd(&out[(size_t)(2 * b) * hg.ND + db], v & 0xffffu);
        if (v >> 16) atomicAdd(&out[(size_t)(2 * b + 1) * hg.ND + db], v >> 16);
    }
}

// one thread per (site, depth bin): the first vs bin of the largest count
__global__ void __launch_bounds__(256) post_argmax_kernel(int S, HistArgs hg, int32_t *argmax)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)S * hg.ND) return;
    const int s = (int)(t / hg.ND), db = (int)(t % hg.ND);
    const int nb = (int)(hg.edge_off[s + 1] - hg.edge_off[s]) - 1;
    const unsigned *cnt = hg.counts + hg.cnt_off[s];
    int best = nb > 0 ? 0 : -1;
    unsigned bv = nb > 0 ? cnt[db] : 0u;
    for (int b = 1; b < nb; ++b) {
        const unsigned v = cnt[(size_t)b * hg.ND + db];
        if (v > bv) { bv = v; best = b; }
    }
    argmax[t] = best;
}

// one lane per kept row: its interface depths over the depth edges; LDS counters when the workgroup's rows are of one site
__global__ void __launch_bounds__(256) post_iface_kernel(int64_t nrows, const int32_t *pn, const int32_t *psite, int ML,
                                                         const double *pd, const float *pdi, const double *edges, int nb,
                                                         unsigned *counts)
{
    __shared__ unsigned h[POST_IFACE_LDS_BINS];
    const int64_t b0 = (int64_t)blockIdx.x * blockDim.x;
    const int64_t r = b0 + threadIdx.x;
    const int64_t rl = (b0 + blockDim.x < nrows ? b0 + blockDim.x : nrows) - 1;
    const bool one = nb <= POST_IFACE_LDS_BINS && psite[b0] == psite[rl];
    if (one) {
        for (int b = threadIdx.x; b < nb; b += blockDim.x) h[b] = 0u;
        __syncthreads();
    }
    if (r < nrows) {
        const int n = pn[r];
        unsigned *out = counts + (size_t)psite[r] * nb;
        for (int j = 0; j < n - 1; ++j) {
            const double v = pdi ? (double)pdi[r * ML + j] : pd[r * ML + j];
            const int b = find_bin(edges, nb, v);
            if (b < 0 || b >= nb) continue;
            if (one) atomicAdd(&h[b], 1u);
            else atomicAdd(&out[b], 1u);
        }
    }
    if (!one) return;
    __syncthreads();
    unsigned *out = counts + (size_t)psite[b0] * nb;
    for (int b = threadIdx.x; b < nb; b += blockDim.x)
        if (h[b]) atomicAdd(&out[b], h[b]);
}

// ---- host side ---------------------------------------------------------------------------------------------------

} // namespace

namespace {

bool grid_ok(const double *dep, int D)
{
    for (int j = 0; j < D; ++j) if (!std::isfinite(dep[j]) || (j && !(dep[j] > dep[j - 1]))) return false;
    return true;
}

ColArgs col_args(bh_posterior *p, const double *dep_d, int D)
{
    ColArgs a;
    a.work = p->dwork.as<PostWork>();
    a.pn = p->pn.as<int32_t>();
    a.pvs = p->pvs.p;
    a.pd = p->pd.as<double>();
    a.ML = p->ML;
    a.D = D;
    a.dep = dep_d;
    return a;
}

int upload_grid(bh_posterior *p, Dev &d, const double *dep, int D)
{
    int rc;
    if (D < 2 || D > (1 << 20) || !dep) return pfail(p, BH_EINVAL, "depth grid: 2..2^20 points");
    if (!grid_ok(dep, D)) return pfail(p, BH_EINVAL, "depth grid must be finite and strictly ascending");
    if ((rc = alloc(p, d, (size_t)D * sizeof(double)))) return rc;
    PCHK(p, hipMemcpyAsync(d.p, dep, (size_t)D * sizeof(double), hipMemcpyHostToDevice, p->st));
    return BH_OK;
}

// the launches of select_ranks over the depth columns: one key width kb for all of them
struct ColSelect {
    bh_posterior *p;
    ColArgs a;
    int kb;
    dim3 grid() const { return dim3((unsigned)p->work.size(), (unsigned)((a.D + 63) / 64)); }
    template <int NR>
    void radix(int R, int pass, const SelectBufs &b) const
    {
        const int shift = kb - 8 * (pass + 1);
        if constexpr (NR == 1) {
            if (p->elem == 4) col_radix1_kernel<float><<<grid(), 64, 0, p->st>>>(a, kb == 32, shift, b.pref, b.ghist);
            else col_radix1_kernel<double><<<grid(), 64, 0, p->st>>>(a, kb == 32, shift, b.pref, b.ghist);
        } else if (p->elem == 4) col_radix_kernel<float, NR><<<grid(), 64, 0, p->st>>>(a, R, kb == 32, shift, b.pref, b.ghist);
        else col_radix_kernel<double, NR><<<grid(), 64, 0, p->st>>>(a, R, kb == 32, shift, b.pref, b.ghist);
    }
    template <int NR>
    void next(int R, const SelectBufs &b) const
    {
        if (p->elem == 4) col_next_kernel<float, NR><<<grid(), 64, 0, p->st>>>(a, R, kb == 32, b.pref, b.nle, b.next);
        else col_next_kernel<double, NR><<<grid(), 64, 0, p->st>>>(a, R, kb == 32, b.pref, b.nle, b.next);
    }
};

// every depth column's count: the rows of its site
std::vector<int64_t> col_counts(const bh_posterior *p, int D)
{
    std::vector<int64_t> n((size_t)p->S * D);
    for (size_t c = 0; c < n.size(); ++c) n[c] = p->off[c / D + 1] - p->off[c / D];
    return n;
}

} // namespace

extern "C" {

int bh_posterior_create(bh_engine *e, bh_posterior **out)
{
    if (!e) return BH_EINVAL;
    if (!out) return bh_engine_fail_internal(e, BH_EINVAL, "null argument");
    bh_posterior *p = new bh_posterior();
    p->e = e;
    p->device = bh_engine_device_internal(e);
    p->st = (hipStream_t)bh_engine_stream(e);
    *out = p;
    return BH_OK;
}

void bh_posterior_destroy(bh_posterior *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    delete p;
}

int bh_posterior_load(bh_posterior *p, int memspace, void *stream, int elem_bytes, int64_t N, int ML, int64_t ld,
                      const void *models, const int32_t *site, int nsites, int64_t *rows, int64_t *invalid, int64_t *dropped)
{
    int rc;
    if (!p) return BH_EINVAL;
    if (elem_bytes != 4 && elem_bytes != 8) return pfail(p, BH_EINVAL, "models must be float32 or float64");
    if (ML < 1 || ML > BH_POSTERIOR_MAXLAYERS)
        return pfail(p, BH_EINVAL, "row width 2*ML must be 2..64 (ML <= BH_POSTERIOR_MAXLAYERS)");
    if (N < 0 || nsites < 1 || nsites > (1 << 20) || ld < 2 * ML) return pfail(p, BH_EINVAL, "bad N, nsites or row stride");
    if ((N && !models) || !rows || !invalid || !dropped) return pfail(p, BH_EINVAL, "null argument");
    PCHK(p, hipSetDevice(p->device));
    const bool host = memspace != BH_DEVICE;
    p->st = (!host && stream) ? (hipStream_t)stream : (hipStream_t)bh_engine_stream(p->e);
    if (host && site)
        for (int64_t r = 0; r < N; ++r)
            if (site[r] < 0 || site[r] >= nsites) return pfail(p, BH_EINVAL, "site index out of range");
    const int S = nsites, W = 2 * ML;
    const size_t eb = (size_t)elem_bytes;
    Dev dm, ds, cnt;
    const void *m = models;
    const int32_t *sd = site;
    if (host && N) {
        if ((rc = alloc(p, dm, (size_t)((N - 1) * ld + W) * eb))) return rc;
        PCHK(p, hipMemcpyAsync(dm.p, models, (size_t)((N - 1) * ld + W) * eb, hipMemcpyHostToDevice, p->st));
        m = dm.p;
        if (site) {
            if ((rc = alloc(p, ds, (size_t)N * sizeof(int32_t)))) return rc;
            PCHK(p, hipMemcpyAsync(ds.p, site, (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, p->st));
            sd = ds.as<int32_t>();
        }
    }
    // counters: rows[S], invalid[S], dropped, not_f32
    const size_t ncnt = 2 * (size_t)S + 2;
    if ((rc = alloc(p, cnt, ncnt * 8))) return rc;
    PCHK(p, hipMemsetAsync(cnt.p, 0, ncnt * 8, p->st));
    unsigned long long *c = cnt.as<unsigned long long>();
    const unsigned nblk = (unsigned)((N + 255) / 256);
    if (N) {
        if (elem_bytes == 4)
            post_count_kernel<float><<<nblk, 256, 0, p->st>>>(N, W, ld, (const float *)m, sd, S, c, c + S, c + 2 * S, (int *)(c + 2 * S + 1));
        else
            post_count_kernel<double><<<nblk, 256, 0, p->st>>>(N, W, ld, (const double *)m, sd, S, c, c + S, c + 2 * S, (int *)(c + 2 * S + 1));
        PCHK(p, hipGetLastError());
    }
    std::vector<unsigned long long> hc(ncnt);
    PCHK(p, hipMemcpyAsync(hc.data(), c, ncnt * 8, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipStreamSynchronize(p->st));
    p->off.assign(S + 1, 0);
    for (int s = 0; s < S; ++s) {
        if (hc[s] >= (1ull << 31)) return pfail(p, BH_EINVAL, "more than 2^31 - 1 rows of one site");
        p->off[s + 1] = p->off[s] + (int64_t)hc[s];
        rows[s] = (int64_t)hc[s];
        invalid[s] = (int64_t)hc[S + s];
    }
    *dropped = (int64_t)hc[2 * S];
    if (host)
        for (int s = 0; s < S; ++s)
            if (hc[S + s]) return pfail(p, BH_EINVAL, "a row's non-NaN values are not a prefix of even length");
    p->elem = elem_bytes;
    p->ML = ML;
    p->S = S;
    p->nrows = p->off[S];
    p->ninput = N;
    for (ScalarSet &ss : p->sets) {  // the sets belong to the rows of the load before
        ss.drop();
        if (ss.val.p) { (void)hipFree(ss.val.p); ss.val.p = nullptr; }
    }
    p->data_filled = -1;
    p->resid_filled = -1;
    p->keys32 = elem_bytes == 4 || (unsigned)hc[2 * S + 1] == 0u;
    const size_t nr = (size_t)p->nrows;
    if ((rc = alloc(p, p->pn, nr * 4))) return rc;
    if ((rc = alloc(p, p->psite, nr * 4))) return rc;
    if ((rc = alloc(p, p->pvs, nr * ML * eb))) return rc;
    if ((rc = alloc(p, p->pd, nr * ML * 8))) return rc;
    p->has_rows = false;
    for (Dev *b : {&p->porig, &p->pzd})   // kept only for the scalar sets: no memory and no writes otherwise
        if (b->p) { (void)hipFree(b->p); b->p = nullptr; }
    if (p->keep_rows && ((rc = alloc(p, p->porig, nr * 8)) || (rc = alloc(p, p->pzd, nr * ML * eb)))) return rc;
    if (elem_bytes == 4) { if ((rc = alloc(p, p->pdi, nr * ML * 4))) return rc; }
    else if (p->pdi.p) { (void)hipFree(p->pdi.p); p->pdi.p = nullptr; }
    // the cursors: each site's first slot
    for (int s = 0; s < S; ++s) hc[s] = (unsigned long long)p->off[s];
    PCHK(p, hipMemcpyAsync(c, hc.data(), (size_t)S * 8, hipMemcpyHostToDevice, p->st));
    if (N) {
        if (elem_bytes == 4)
            post_scatter_kernel<float><<<nblk, 256, 0, p->st>>>(N, W, ld, (const float *)m, sd, S, ML, c, p->pn.as<int32_t>(),
                p->psite.as<int32_t>(), p->pvs.as<float>(), p->pd.as<double>(), p->pdi.as<float>(), p->porig.as<int64_t>(), p->pzd.as<float>());
        else
            post_scatter_kernel<double><<<nblk, 256, 0, p->st>>>(N, W, ld, (const double *)m, sd, S, ML, c, p->pn.as<int32_t>(),
                p->psite.as<int32_t>(), p->pvs.as<double>(), p->pd.as<double>(), nullptr, p->porig.as<int64_t>(), p->pzd.as<double>());
        PCHK(p, hipGetLastError());
    }
    p->work.clear();
    for (int s = 0; s < S; ++s)
        for (int64_t r = p->off[s]; r < p->off[s + 1]; r += POST_CHUNK)
            p->work.push_back(PostWork{s, 0, r, std::min<int64_t>(r + POST_CHUNK, p->off[s + 1])});
    if ((rc = alloc(p, p->dwork, p->work.size() * sizeof(PostWork)))) return rc;
    if (!p->work.empty())
        PCHK(p, hipMemcpyAsync(p->dwork.p, p->work.data(), p->work.size() * sizeof(PostWork), hipMemcpyHostToDevice, p->st));
    PCHK(p, hipStreamSynchronize(p->st));
    p->has_rows = p->keep_rows;
    return BH_OK;
}

int bh_posterior_columns(bh_posterior *p, int D, const double *dep, uint64_t *kmin, uint64_t *kmax, int32_t *scale,
                         int64_t *x0, int32_t *exact, uint64_t *sums, uint64_t *median, int32_t *keys32)
{
    int rc;
    if (!p) return BH_EINVAL;
    if (p->S < 1) return pfail(p, BH_EINVAL, "no rows loaded (bh_posterior_load)");
    if (!kmin || !kmax || !scale || !x0 || !exact || !sums || !keys32) return pfail(p, BH_EINVAL, "null argument");
    PCHK(p, hipSetDevice(p->device));
    Dev dd, dmin, dmax, dlow, dsc, dx0, dsum;
    if ((rc = upload_grid(p, dd, dep, D))) return rc;
    const size_t ncol = (size_t)p->S * D;
    if ((rc = alloc(p, dmin, ncol * 8)) || (rc = alloc(p, dmax, ncol * 8)) || (rc = alloc(p, dlow, ncol * 4))) return rc;
    PCHK(p, hipMemsetAsync(dmin.p, 0xff, ncol * 8, p->st));
    PCHK(p, hipMemsetAsync(dmax.p, 0, ncol * 8, p->st));
    PCHK(p, hipMemsetAsync(dlow.p, 0x7f, ncol * 4, p->st)); // 0x7f7f7f7f: above every exponent
    const ColArgs a = col_args(p, dd.as<double>(), D);
    const dim3 grid((unsigned)p->work.size(), (unsigned)((D + 63) / 64));
    const bool f = p->elem == 4;
    if (!p->work.empty()) {
        if (f) post_stats_kernel<float><<<grid, 64, 0, p->st>>>(a, dmin.as<unsigned long long>(), dmax.as<unsigned long long>(), dlow.as<int>());
        else post_stats_kernel<double><<<grid, 64, 0, p->st>>>(a, dmin.as<unsigned long long>(), dmax.as<unsigned long long>(), dlow.as<int>());
        PCHK(p, hipGetLastError());
    }
    std::vector<int32_t> low(ncol);
    PCHK(p, hipMemcpyAsync(kmin, dmin.p, ncol * 8, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipMemcpyAsync(kmax, dmax.p, ncol * 8, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipMemcpyAsync(low.data(), dlow.p, ncol * 4, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipStreamSynchronize(p->st));
    const std::vector<int64_t> count = col_counts(p, D);
    for (size_t c = 0; c < ncol; ++c) {   // the fixed-point scale of every column
        if (count[c] == 0) { scale[c] = 0; x0[c] = 0; exact[c] = 1; continue; }
        if ((rc = scale_rule(p, kmin[c], kmax[c], low[c], "a velocity is not finite", &scale[c], &x0[c], &exact[c]))) return rc;
    }
    if ((rc = alloc(p, dsc, ncol * 4)) || (rc = alloc(p, dx0, ncol * 8)) || (rc = alloc(p, dsum, ncol * 48))) return rc;
    PCHK(p, hipMemcpyAsync(dsc.p, scale, ncol * 4, hipMemcpyHostToDevice, p->st));
    PCHK(p, hipMemcpyAsync(dx0.p, x0, ncol * 8, hipMemcpyHostToDevice, p->st));
    PCHK(p, hipMemsetAsync(dsum.p, 0, ncol * 48, p->st));
    if (!p->work.empty()) {
        if (f) post_moments_kernel<float><<<grid, 64, 0, p->st>>>(a, dsc.as<int32_t>(), dx0.as<int64_t>(), dsum.as<unsigned long long>());
        else post_moments_kernel<double><<<grid, 64, 0, p->st>>>(a, dsc.as<int32_t>(), dx0.as<int64_t>(), dsum.as<unsigned long long>());
        PCHK(p, hipGetLastError());
    }
    PCHK(p, hipMemcpyAsync(sums, dsum.p, ncol * 48, hipMemcpyDeviceToHost, p->st));
    *keys32 = p->keys32 ? 1 : 0;
    if (median) {   // the keys of ranks (n-1)/2 and (n-1)/2 + 1, in the width keys32 tells
        std::vector<uint32_t> rk(ncol);
        for (size_t c = 0; c < ncol; ++c) rk[c] = count[c] ? (uint32_t)((count[c] - 1) / 2) : 0u;
        const int kb = p->keys32 ? 32 : 64;
        if ((rc = select_ranks(p, ncol, 1, rk.data(), count.data(), {kb}, false, ColSelect{p, a, kb}, median, median + 1, 2))) return rc;
    }
    PCHK(p, hipStreamSynchronize(p->st));
    return BH_OK;
}

int bh_posterior_column_quantiles(bh_posterior *p, int D, const double *dep, int R, const uint32_t *rank, uint64_t *lower,
                                  uint64_t *upper, int32_t *keys32)
{
    int rc;
    if (!p) return BH_EINVAL;
    if (p->S < 1) return pfail(p, BH_EINVAL, "no rows loaded (bh_posterior_load)");
    if (R < 1 || R > SELECT_MAXR) return pfail(p, BH_EINVAL, "ranks per column: 1..BH_QUANTILES_MAXRANKS");
    if (!dep || !rank || !lower || !upper) return pfail(p, BH_EINVAL, "null argument");
    if (D < 1 || D > (1 << 20)) return pfail(p, BH_EINVAL, "depth grid: 1..2^20 points");
    if (!grid_ok(dep, D)) return pfail(p, BH_EINVAL, "depth grid must be finite and strictly ascending");
    const int S = p->S;
    for (int s = 0; s < S; ++s) {
        const int64_t n = p->off[s + 1] - p->off[s];
        if (n >= (1ll << 32)) return pfail(p, BH_EUNSUPPORTED, "2^32 or more rows of one site");
        for (int r = 0; r < R; ++r)
            if ((int64_t)rank[(size_t)s * R + r] >= std::max<int64_t>(n, 1)) return pfail(p, BH_EINVAL, "a rank is not below its site's rows");
    }
    PCHK(p, hipSetDevice(p->device));
    const size_t ncol = (size_t)S * D;
    Dev dd;
    if ((rc = alloc(p, dd, (size_t)D * sizeof(double)))) return rc;
    std::vector<uint32_t> rk(ncol * R);
    for (size_t c = 0; c < ncol; ++c)
        for (int r = 0; r < R; ++r) rk[c * R + r] = rank[(c / D) * R + r];
    PCHK(p, hipMemcpyAsync(dd.p, dep, (size_t)D * sizeof(double), hipMemcpyHostToDevice, p->st));
    const int kb = p->keys32 ? 32 : 64;
    const ColSelect launch{p, col_args(p, dd.as<double>(), D), kb};
    if ((rc = select_ranks(p, ncol, R, rk.data(), col_counts(p, D).data(), {kb}, false, launch, lower, upper, 1))) return rc;
    if (keys32) *keys32 = p->keys32 ? 1 : 0;
    return BH_OK;
}

int bh_posterior_hist(bh_posterior *p, int D, const double *dep, const int32_t *dbin, int ND, const int64_t *edge_off,
                      const double *edges, uint32_t *counts, int32_t *argmax)
{
    int rc;
    if (!p) return BH_EINVAL;
    if (p->S < 1) return pfail(p, BH_EINVAL, "no rows loaded (bh_posterior_load)");
    if (!dbin || !edge_off || !edges || !counts) return pfail(p, BH_EINVAL, "null argument");
    if (ND < 1 || ND > (1 << 20)) return pfail(p, BH_EINVAL, "depth bins: 1..2^20");
    for (int j = 0; j < D; ++j)
        if (dbin[j] < -1 || dbin[j] >= ND) return pfail(p, BH_EINVAL, "depth bin index out of range");
    const int S = p->S;
    if (edge_off[0] != 0) return pfail(p, BH_EINVAL, "edge offsets must start at 0");
    std::vector<int64_t> coff(S);
    int64_t ncells = 0;
    int maxnb = 0;
    for (int s = 0; s < S; ++s) {
        const int64_t nb = edge_off[s + 1] - edge_off[s] - 1;
        if (nb < 1) return pfail(p, BH_EINVAL, "every site needs at least 2 vs edges");
        for (int64_t i = edge_off[s]; i <= edge_off[s] + nb; ++i)
            if (!std::isfinite(edges[i]) || (i > edge_off[s] && edges[i] < edges[i - 1]))
                return pfail(p, BH_EINVAL, "vs edges must be finite and ascending");
        coff[s] = ncells;
        if (nb > (int64_t)BH_POSTERIOR_MAXCOUNTS / ND || ncells + nb * ND > (int64_t)BH_POSTERIOR_MAXCOUNTS)
            return pfail(p, BH_EINVAL, "the histogram would exceed BH_POSTERIOR_MAXCOUNTS (2^27) cells: is the vs range sane?");
        ncells += nb * ND;
        maxnb = std::max<int>(maxnb, (int)nb);
    }
    PCHK(p, hipSetDevice(p->device));
    Dev dd, ddb, deo, ded, dco, dcnt, dam;
    if ((rc = upload_grid(p, dd, dep, D))) return rc;
    const size_t ne = (size_t)edge_off[S];
    if ((rc = alloc(p, ddb, (size_t)D * 4)) || (rc = alloc(p, deo, (size_t)(S + 1) * 8)) || (rc = alloc(p, ded, ne * 8)) ||
        (rc = alloc(p, dco, (size_t)S * 8)) || (rc = alloc(p, dcnt, (size_t)ncells * 4)))
        return rc;
    PCHK(p, hipMemcpyAsync(ddb.p, dbin, (size_t)D * 4, hipMemcpyHostToDevice, p->st));
    PCHK(p, hipMemcpyAsync(deo.p, edge_off, (size_t)(S + 1) * 8, hipMemcpyHostToDevice, p->st));
    PCHK(p, hipMemcpyAsync(ded.p, edges, ne * 8, hipMemcpyHostToDevice, p->st));
    PCHK(p, hipMemcpyAsync(dco.p, coff.data(), (size_t)S * 8, hipMemcpyHostToDevice, p->st));
    PCHK(p, hipMemsetAsync(dcnt.p, 0, (size_t)ncells * 4, p->st));
    HistArgs hg;
    hg.dbin = ddb.as<int32_t>();
    hg.ND = ND;
    hg.edge_off = deo.as<int64_t>();
    hg.edges = ded.as<double>();
    hg.cnt_off = dco.as<int64_t>();
    hg.counts = dcnt.as<unsigned>();
    hg.lds = maxnb <= POST_HIST_LDS_BINS;
    const ColArgs a = col_args(p, dd.as<double>(), D);
    const dim3 grid((unsigned)p->work.size(), (unsigned)((D + 63) / 64));
    if (!p->work.empty()) {
        if (p->elem == 4) post_hist_kernel<float><<<grid, 64, 0, p->st>>>(a, hg);
        else post_hist_kernel<double><<<grid, 64, 0, p->st>>>(a, hg);
        PCHK(p, hipGetLastError());
    }
    if (argmax) {
        if ((rc = alloc(p, dam, (size_t)S * ND * 4))) return rc;
        post_argmax_kernel<<<(unsigned)(((int64_t)S * ND + 255) / 256), 256, 0, p->st>>>(S, hg, dam.as<int32_t>());
        PCHK(p, hipGetLastError());
        PCHK(p, hipMemcpyAsync(argmax, dam.p, (size_t)S * ND * 4, hipMemcpyDeviceToHost, p->st));
    }
    PCHK(p, hipMemcpyAsync(counts, dcnt.p, (size_t)ncells * 4, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipStreamSynchronize(p->st));
    return BH_OK;
}

int bh_posterior_interfaces(bh_posterior *p, int nedges, const double *edges, uint32_t *counts)
{
    int rc;
    if (!p) return BH_EINVAL;
    if (p->S < 1) return pfail(p, BH_EINVAL, "no rows loaded (bh_posterior_load)");
    if (!edges || !counts) return pfail(p, BH_EINVAL, "null argument");
    if (nedges < 2 || nedges > (1 << 24)) return pfail(p, BH_EINVAL, "depth edges: 2..2^24");
    for (int i = 0; i < nedges; ++i)
        if (!std::isfinite(edges[i]) || (i && edges[i] < edges[i - 1])) return pfail(p, BH_EINVAL, "depth edges must be finite and ascending");
    const int nb = nedges - 1;
    if ((int64_t)p->S * nb > (int64_t)BH_POSTERIOR_MAXCOUNTS)
        return pfail(p, BH_EINVAL, "the histogram would exceed BH_POSTERIOR_MAXCOUNTS (2^27) cells");
    PCHK(p, hipSetDevice(p->device));
    Dev ded, dcnt;
    const size_t ncells = (size_t)p->S * nb;
    if ((rc = alloc(p, ded, (size_t)nedges * 8)) || (rc = alloc(p, dcnt, ncells * 4))) return rc;
    PCHK(p, hipMemcpyAsync(ded.p, edges, (size_t)nedges * 8, hipMemcpyHostToDevice, p->st));
    PCHK(p, hipMemsetAsync(dcnt.p, 0, ncells * 4, p->st));
    if (p->nrows) {
        const unsigned nblk = (unsigned)((p->nrows + 255) / 256);
        post_iface_kernel<<<nblk, 256, 0, p->st>>>(p->nrows, p->pn.as<int32_t>(), p->psite.as<int32_t>(), p->ML,
                                                          p->pd.as<double>(), p->pdi.as<float>(), ded.as<double>(), nb, dcnt.as<unsigned>());
        PCHK(p, hipGetLastError());
    }
    PCHK(p, hipMemcpyAsync(counts, dcnt.p, ncells * 4, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipStreamSynchronize(p->st));
    return BH_OK;
}

} // extern "C"
