// bayhunter_amd/csrc/posterior_select.h -- the order statistics of the posterior summaries: one 8-bit radix select over ordered keys
// for the medians and quantiles of posterior_kernel.hip, posterior_scalars_kernel.hip and posterior_datafit_kernel.hip, and the
// small helpers these files (and posterior_cov_kernel.hip) share.
//
// A select finds R ranks per column.  Per pass every key is counted by its 8-bit digit for the rank whose prefix it matches
// (radix), one thread per column picks every rank's digit (pick), and a last pass finds per rank the number of keys <= the
// selected one and the least key above it (next).  Prefixes, ranks and counters lie at [column * R + rank].  Ranks whose prefixes
// are still equal share the counters of the first of them, their owner.
//   radix, next : per source layout -- col_radix_kernel / col_next_kernel (posterior_kernel.hip: a lane per depth column, rows
//                 sampled) and set_radix_kernel / set_next_kernel (here: 256 lanes stride over the rows of a scalar column)
//   pick        : select_pick_kernel, one for both
// Every kernel is a template on the rank capacity NR and is instantiated with NR = 1 (a median, or one rank: the owner mask is
// constant and there is no lead search) and NR = BH_QUANTILES_MAXRANKS; only the column layout's radix pass of one rank is
// written out (col_radix1_kernel, posterior_kernel.hip: the instantiation measured slower).  The kernels have internal
// linkage: every translation unit that selects holds its own instantiations.  select_ranks is the one host driver.
#ifndef BH_POSTERIOR_SELECT_H
#define BH_POSTERIOR_SELECT_H

#include "posterior_common.h"
#include "../../include/bh_engine_posterior_datafit.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#define SELECT_MAXR BH_QUANTILES_MAXRANKS
#define SET_THREADS 256   // lanes of a workgroup of a pass over a scalar set

namespace bhpost {

__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7ff8000000000000ll); }

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long wave_min(unsigned long long v)
{
    for (int o = 32; o; o >>= 1) { const unsigned long long u = __shfl_xor(v, o); v = u < v ? u : v; }
    return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v)
{
    for (int o = 32; o; o >>= 1) { const unsigned long long u = __shfl_xor(v, o); v = u > v ? u : v; }
    return v;
}
__device__ __forceinline__ int wave_min_i(int v)
{
    for (int o = 32; o; o >>= 1) { const int u = __shfl_xor(v, o); v = u < v ? u : v; }
    return v;
}

// the 64-bit ordered key of the float32 value behind a 32-bit ordered key (bh_okey.h)
inline uint64_t widen_key(uint64_t k32) { return okey64((double)okey32_value((uint32_t)k32)); }

// the fixed-point scale of a column with values, from its least and largest key and its lowest set bit: the lowest set bit,
// raised until |X| < 2^62; x0 = the least value at that scale.  A value that is not finite is refused with the caller's text.
inline int scale_rule(bh_posterior *p, uint64_t kmin, uint64_t kmax, int low, const char *not_finite, int32_t *scale, int64_t *x0,
                      int32_t *exact)
{
    const double vmn = okey64_value(kmin), vmx = okey64_value(kmax);
    const double amax = std::max(std::fabs(vmn), std::fabs(vmx));
    if (!std::isfinite(amax)) return pfail(p, BH_EINVAL, not_finite);
    int L = 0;
    *exact = 1;
    if (amax > 0.0) {
        int ea;
        (void)std::frexp(amax, &ea); // amax < 2^ea
        L = std::max(low, ea - 62);
        *exact = low >= ea - 62;
    }
    *scale = L;
    *x0 = (int64_t)std::nearbyint(std::ldexp(vmn, -L));
    return BH_OK;
}

struct SetArgs {
    const PostWork *work;
    const double *val;
    int64_t nrows;
    int Q;
};

inline int get_set(bh_posterior *p, int set, ScalarSet **out)
{
    if (p->S < 1) return pfail(p, BH_EINVAL, "no rows loaded (bh_posterior_load)");
    const int slot = set_slot(set);
    if (slot < 0) return pfail(p, BH_EINVAL, "no such scalar set");
    if (p->sets[slot].Q < 1)
        return pfail(p, BH_EINVAL, slot == 0   ? "the MOHO set does not exist yet (bh_posterior_moho)"
                                   : slot == 1 ? "the USER set does not exist yet (bh_posterior_attach)"
                                   : slot == 2 ? "the DATA set does not exist yet (bh_posterior_data_fill over all rows)"
                                   : slot == 3 ? "the FEATURES set does not exist yet (bh_posterior_features)"
                                               : "the RESID set does not exist yet (bh_posterior_resid_fill over all rows)");
    *out = &p->sets[slot];
    return BH_OK;
}

inline SetArgs set_args(bh_posterior *p, const ScalarSet *ss)
{
    SetArgs a;
    a.work = p->dwork.as<PostWork>();
    a.val = ss->val.as<double>();
    a.nrows = p->nrows;
    a.Q = ss->Q;
    return a;
}

// ---- the select: what its kernels share ---------------------------------------------------------------------------

// the ranks of a call: a compile-time 1 where the capacity is 1
template <int NR>
__device__ __forceinline__ int select_ranks_of(int R) { return NR == 1 ? 1 : R; }

template <int NR>
__device__ __forceinline__ void load_prefixes(unsigned long long (&p)[NR], const unsigned long long *pref, int R)
{
#pragma unroll
    for (int r = 0; r < NR; ++r) p[r] = r < R ? pref[r] : 0ull;
}

// key k lies under prefix p above bit hs (hs >= 64: the first pass, no prefix yet -- and no shift by the key's whole width)
__device__ __forceinline__ bool key_matches(unsigned long long k, unsigned long long p, int hs)
{
    return hs >= 64 || ((k ^ p) >> hs) == 0ull;
}

__device__ __forceinline__ unsigned key_digit(unsigned long long k, int shift) { return (unsigned)(k >> shift) & 255u; }

// the first rank of 0..r whose prefix above bit hs equals r's: it owns the counters r reads
template <int NR>
__device__ __forceinline__ int lead_rank(const unsigned long long (&p)[NR], int r, int R, int hs)
{
    int lead = r;
#pragma unroll
    for (int r2 = NR - 1; r2 >= 0; --r2)
        if (r2 < r && r2 < R && key_matches(p[r2], p[r], hs)) lead = r2;
    return lead;
}

// bit r: rank r owns its counters (the owners' prefixes differ, so a key matches at most one of them; rank 0 always owns)
template <int NR>
__device__ __forceinline__ unsigned owner_mask(const unsigned long long (&p)[NR], int R, int hs)
{
    unsigned own = 0u;
#pragma unroll
    for (int r = 0; r < NR; ++r) own |= (r < R && lead_rank<NR>(p, r, R, hs) == r) ? 1u << r : 0u;
    return own;
}

namespace {

// one thread per column: per rank the digit at kbits[c % Q] - 8 * (pass + 1) holding it, read from the counters of the rank that
// owns them; then the counters are cleared for the next pass (columns with fewer passes sit the later ones out)
template <int NR>
__global__ void __launch_bounds__(256) select_pick_kernel(size_t ncol, int Q, int Rarg, const int *kbits, int pass, unsigned *ghist,
                                                          unsigned long long *pref, unsigned *rank)
{
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncol) return;
    const int R = select_ranks_of<NR>(Rarg);
    const int shift = kbits[c % Q] - 8 * (pass + 1);
    if (shift < 0) return;
    const int hs = shift + 8;
    unsigned long long p[NR];
    int dgs[NR];
    unsigned rest[NR];
    load_prefixes<NR>(p, pref + c * R, R);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        dgs[r] = -1;
        rest[r] = 0u;
        if (r >= R) continue;
        unsigned *g = ghist + (c * R + lead_rank<NR>(p, r, R, hs)) * 256;
        const unsigned k = rank[c * R + r];
        unsigned cum = 0;
        int dg = -1;
        for (int b = 0; b < 256; ++b) {
            const unsigned hb = g[b];
            if (dg < 0 && k < cum + hb) dg = b;
            if (dg < 0) cum += hb;
            if (NR == 1) g[b] = 0u; // one rank: nobody else reads its counters, cleared as they are read
        }
        dgs[r] = dg;
        rest[r] = k - cum;
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        if (r >= R) continue;
        unsigned *g = ghist + (c * R + r) * 256;
        if (NR > 1)
            for (int b = 0; b < 256; ++b) g[b] = 0u;
        if (dgs[r] < 0) continue; // a column without rows (a depth column) / a column without values (a scalar column)
        rank[c * R + r] = rest[r];
        pref[c * R + r] = p[r] | ((unsigned long long)dgs[r] << shift);
    }
}

// pass `pass` of the select over a scalar set: per (site, column, rank) the histogram of the 8-bit digit at kbits[q] - 8 * (pass +
// 1) over the keys that match the rank's prefix above it: 256 LDS counters per rank, a key counted for the owner it matches
// (pass 0 costs one LDS atomic per key whatever R is)
template <int NR>
__global__ void __launch_bounds__(SET_THREADS) set_radix_kernel(SetArgs a, int Rarg, const int *kbits, int pass,
                                                                const unsigned long long *pref, unsigned *ghist)
{
    __shared__ unsigned h[NR * 256];
    const PostWork w = a.work[blockIdx.x];
    const int q = blockIdx.y;
    const int kb = kbits[q];
    const int shift = kb - 8 * (pass + 1);
    if (shift < 0) return; // (uniform over the workgroup: before the barriers)
    const int R = select_ranks_of<NR>(Rarg);
    const int hs = shift + 8;
    const size_t c = (size_t)w.site * a.Q + q;
    unsigned long long p[NR];
    load_prefixes<NR>(p, pref + c * R, R);
    const unsigned own = owner_mask<NR>(p, R, hs);
#pragma unroll
    for (int r = 0; r < NR; ++r)
        if (r < R) h[r * 256 + threadIdx.x] = 0u;   // SET_THREADS == 256
    __syncthreads();
    const double *col = a.val + (int64_t)q * a.nrows;
    for (int64_t i = w.r0 + threadIdx.x; i < w.r1; i += SET_THREADS) {
        const double v = col[i];
        if (v != v) continue;
        const unsigned long long k = okey(v, kb == 32);
        const unsigned dg = key_digit(k, shift);
#pragma unroll
        for (int r = 0; r < NR; ++r)
            if (((own >> r) & 1u) && key_matches(k, p[r], hs)) atomicAdd(&h[r * 256 + dg], 1u);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        if (!((own >> r) & 1u)) continue;
        const unsigned v = h[r * 256 + threadIdx.x];
        if (v) atomicAdd(&ghist[(c * R + r) * 256 + threadIdx.x], v);
    }
}

// per rank the number of keys <= the selected one, and the least key above it
template <int NR>
__global__ void __launch_bounds__(SET_THREADS) set_next_kernel(SetArgs a, int Rarg, const int *kbits, const unsigned long long *pref,
                                                               unsigned *nle, unsigned long long *next)
{
    const PostWork w = a.work[blockIdx.x];
    const int q = blockIdx.y;
    const int R = select_ranks_of<NR>(Rarg);
    const size_t c = (size_t)w.site * a.Q + q;
    const double *col = a.val + (int64_t)q * a.nrows;
    const bool k32 = kbits[q] == 32;
    unsigned long long p[NR], le[NR], nx[NR];
    load_prefixes<NR>(p, pref + c * R, R);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        le[r] = 0ull;
        nx[r] = ~0ull;
    }
    for (int64_t i = w.r0 + threadIdx.x; i < w.r1; i += SET_THREADS) {
        const double v = col[i];
        if (v != v) continue;
        const unsigned long long k = okey(v, k32);
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            le[r] += k <= p[r] ? 1u : 0u;
            nx[r] = (k > p[r] && k < nx[r]) ? k : nx[r];
        }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        if (r >= R) continue;   // (uniform)
        const unsigned long long l = wave_sum(le[r]), n = wave_min(nx[r]);
        if (__lane_id() == 0) {
            if (l) atomicAdd(&nle[c * R + r], (unsigned)l);
            atomicMin(&next[c * R + r], n);
        }
    }
}

// ---- the select: its host driver (internal as well: it launches this translation unit's kernels) ------------------

struct SelectBufs {
    const int *kbits;         // [Q]
    unsigned long long *pref; // [ncol * R]
    unsigned *ghist;          // [ncol * R * 256]
    unsigned *nle;            // [ncol * R]
    unsigned long long *next; // [ncol * R]
};

// the launches of the radix and the next pass over a scalar set (the column layout's: posterior_kernel.hip)
struct SetSelect {
    bh_posterior *p;
    SetArgs a;
    template <int NR>
    void radix(int R, int pass, const SelectBufs &b) const
    {
        set_radix_kernel<NR><<<dim3((unsigned)p->work.size(), (unsigned)a.Q), SET_THREADS, 0, p->st>>>(a, R, b.kbits, pass, b.pref, b.ghist);
    }
    template <int NR>
    void next(int R, const SelectBufs &b) const
    {
        set_next_kernel<NR><<<dim3((unsigned)p->work.size(), (unsigned)a.Q), SET_THREADS, 0, p->st>>>(a, R, b.kbits, b.pref, b.nle, b.next);
    }
};

template <int NR, typename Launch>
void select_passes(bh_posterior *p, size_t ncol, int Q, int R, int passes, const Launch &launch, const SelectBufs &b, unsigned *rank)
{
    const unsigned pb = (unsigned)((ncol + 255) / 256);
    for (int pass = 0; pass < passes; ++pass) {
        launch.template radix<NR>(R, pass, b);
        select_pick_kernel<NR><<<pb, 256, 0, p->st>>>(ncol, Q, R, b.kbits, pass, b.ghist, b.pref, rank);
    }
    launch.template next<NR>(R, b);
}

// R order statistics of every column: rank [ncol * R] (each below its column's count), count [ncol], kbits [Q] the key width of
// column c % Q (32: float32-exact values, 4 passes; 64: 8 passes), launch the layout's radix and next pass.  lower / upper
// [(c * R + r) * ostride]: the keys of rank and rank + 1 (the last key again past the end), 32-bit keys widened where asked;
// zero for a column without values.
template <typename Launch>
int select_ranks(bh_posterior *p, size_t ncol, int R, const uint32_t *rank, const int64_t *count, const std::vector<int> &kbits,
                 bool widen, const Launch &launch, uint64_t *lower, uint64_t *upper, size_t ostride)
{
    int rc;
    const size_t nr = ncol * R;
    const int Q = (int)kbits.size();
    Dev dh, dpref, drank, dnle, dnext, dkb;
    if ((rc = alloc(p, dh, nr * 256 * 4)) || (rc = alloc(p, dpref, nr * 8)) || (rc = alloc(p, drank, nr * 4)) ||
        (rc = alloc(p, dnle, nr * 4)) || (rc = alloc(p, dnext, nr * 8)) || (rc = alloc(p, dkb, (size_t)Q * 4)))
        return rc;
    PCHK(p, hipMemsetAsync(dh.p, 0, nr * 256 * 4, p->st));
    PCHK(p, hipMemsetAsync(dpref.p, 0, nr * 8, p->st));
    PCHK(p, hipMemsetAsync(dnle.p, 0, nr * 4, p->st));
    PCHK(p, hipMemsetAsync(dnext.p, 0xff, nr * 8, p->st));
    PCHK(p, hipMemcpyAsync(drank.p, rank, nr * 4, hipMemcpyHostToDevice, p->st));
    PCHK(p, hipMemcpyAsync(dkb.p, kbits.data(), (size_t)Q * 4, hipMemcpyHostToDevice, p->st));
    if (!p->work.empty()) {
        const SelectBufs b{dkb.as<int>(), dpref.as<unsigned long long>(), dh.as<unsigned>(), dnle.as<unsigned>(), dnext.as<unsigned long long>()};
        const int passes = *std::max_element(kbits.begin(), kbits.end()) / 8;
        if (R == 1) select_passes<1>(p, ncol, Q, R, passes, launch, b, drank.as<unsigned>());
        else select_passes<SELECT_MAXR>(p, ncol, Q, R, passes, launch, b, drank.as<unsigned>());
        PCHK(p, hipGetLastError());
    }
    std::vector<uint64_t> pref(nr), next(nr);
    std::vector<unsigned> nle(nr);
    PCHK(p, hipMemcpyAsync(pref.data(), dpref.p, nr * 8, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipMemcpyAsync(next.data(), dnext.p, nr * 8, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipMemcpyAsync(nle.data(), dnle.p, nr * 4, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipStreamSynchronize(p->st));
    for (size_t i = 0; i < nr; ++i) {
        const size_t c = i / R;
        if (count[c] == 0) { lower[i * ostride] = upper[i * ostride] = 0; continue; }
        // rank + 1 is the selected key again while more keys than rank + 1 are <= it
        const uint64_t up = ((uint64_t)nle[i] >= (uint64_t)rank[i] + 2u || next[i] == ~0ull) ? pref[i] : next[i];
        const bool w = widen && kbits[c % Q] == 32;
        lower[i * ostride] = w ? widen_key(pref[i]) : pref[i];
        upper[i * ostride] = w ? widen_key(up) : up;
    }
    return BH_OK;
}

} // namespace
} // namespace bhpost
#endif
