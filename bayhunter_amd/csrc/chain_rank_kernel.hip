// bayhunter_amd/csrc/chain_rank_kernel.hip -- the rank transform of the chains' recorded series (include/bh_engine_chain_rank.h).
//
// The pool of (group g, column q) is the N_g = m_g * T values of the group's kept chains.  The pools of one column lie one after
// the other in the scratch buffers (segment g at seg_base[g]); a segment is cut into tiles of BH_RANK_TILE keys, one workgroup
// each.  The call walks the columns; per column:
//   extract : element (t, c) of every kept chain -> its order-preserving unsigned key (32-bit for float32 tables, 64-bit for
//             float64) and its element index t*C + c.  Model rows give their values through chain_diag_value.h.
//   sort    : least-significant-digit radix sort of every segment, 8 bits per pass, three launches per pass:
//             hist    -- per tile the 256 digit counts (LDS);
//             scan    -- per segment: thread d runs over the tiles' counts of digit d (exclusive), then the digits' totals;
//             scatter -- a tile's keys, in steps of 256 in their order, each to  digit base + tile base + rank among the tile's
//                        equal digits before it: the pass is stable, which is what an LSD sort needs of it.
//             Equal digits of a wavefront are found with eight 64-bit ballots (one per digit bit); a lane's rank is the count of
//             lower lanes in its match mask, the lowest lane of a mask carries the count.  No LDS atomic is contended by a whole
//             wavefront: a column whose keys share a digit (a constant, a likelihood near -1e4) costs what any other does.
//   write   : position i of a sorted segment: lt = the start of its tie run, eq the run's length -- both neighbours differ: the
//             position itself; else a binary search in the sorted segment --, R2 = 2 lt + eq + 1, z = zt[zoff + R2], the tail
//             indicators from lt, all stored at the element's place in the outputs (plain vector stores).
//   fold    : med from the two middle keys of a sorted segment, f = |v - med| -> 64-bit keys at the same positions, sorted
//             again (8 passes), written as zf.
// Every output is a function of integer counts: the order in which atomics land changes nothing.
#include "bh_hostkit.h"
#include "bh_okey.h"
#include "chain_diag_value.h"
#include "chain_tables.h"
#include "../../include/bh_engine_chain_rank.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#pragma clang fp contract(off)

#define RANK_TILE BH_RANK_TILE
#define RANK_FINITE 1.7976931348623157e308

static_assert(BH_RANK_RADIXBITS == 8 && RANK_TILE % 256 == 0, "a pass: 256 digits, 256 threads, tiles of whole steps");

namespace {

using namespace bhkit;

// the pools of a call (device arrays)
struct Pools {
    const unsigned *seg_base;   // [G+1] first position of a segment
    const int *seg_m;           // [G]   kept chains of the group
    const int *seg_moff;        // [G]   its first entry of member
    const int *seg_blk0;        // [G+1] its first tile
    const int *member;          // the kept chains, group by group
    const int *blk_seg;         // [tiles] the segment of a tile
};

struct RankArgs {
    const void *x;
    int64_t T, ld_t, ld_c;
    int C, ML, D;
    const double *dep;          // device [D] (models)
    Pools p;
};

// the tile of this workgroup: its segment, the positions [lo, hi) it covers and the segment's [s0, s1)
struct Tile {
    int g;
    unsigned s0, s1, lo, hi;
};
__device__ __forceinline__ Tile tile_of(const Pools &p, int blk)
{
    Tile t;
    t.g = p.blk_seg[blk];
    t.s0 = p.seg_base[t.g];
    t.s1 = p.seg_base[t.g + 1];
    const unsigned long long lo = (unsigned long long)t.s0 + (unsigned long long)(blk - p.seg_blk0[t.g]) * RANK_TILE;
    const unsigned long long hi = lo + RANK_TILE;
    t.lo = (unsigned)lo;
    t.hi = hi < t.s1 ? (unsigned)hi : t.s1;
    return t;
}

// the row of pool position pos of tile t: element e = pos - s0 is (row e / m, the group's chain e % m)
template <typename T>
__device__ __forceinline__ const T *row_of(const RankArgs &a, const Tile &t, unsigned pos, unsigned &elem)
{
    const unsigned e = pos - t.s0, m = (unsigned)a.p.seg_m[t.g];
    const unsigned row = e / m, j = e - row * m;
    const int c = a.p.member[a.p.seg_moff[t.g] + (int)j];
    elem = row * (unsigned)a.C + (unsigned)c;
    return (const T *)a.x + (int64_t)row * a.ld_t + (int64_t)c * a.ld_c;
}

// every value of the kept chains, all columns: flag |= 1 a value that is not finite, |= 2 a model row that is not a row
template <typename T, bool MODELS>
__global__ void __launch_bounds__(256) rank_check_kernel(RankArgs a, int Q, int *flag)
{
    const Tile t = tile_of(a.p, blockIdx.x);
    int bad = 0;
    for (unsigned pos = t.lo + threadIdx.x; pos < t.hi; pos += 256) {
        unsigned elem;
        const T *row = row_of<T>(a, t, pos, elem);
        if (MODELS) {
            (void)diag_model_value<T, true>(row, a.ML, a.D, a.dep, a.D, RANK_FINITE, bad);
        } else {
            for (int q = 0; q < Q; ++q)
                if (!(fabs((double)row[q]) <= RANK_FINITE)) bad |= 1;
        }
    }
    if (bad) atomicOr(flag, bad);
}

template <typename T, bool MODELS>
__global__ void __launch_bounds__(256) rank_extract_kernel(RankArgs a, int q, okey_t<T> *keys, unsigned *idx)
{
    const Tile t = tile_of(a.p, blockIdx.x);
    for (unsigned pos = t.lo + threadIdx.x; pos < t.hi; pos += 256) {
        unsigned elem;
        const T *row = row_of<T>(a, t, pos, elem);
        int dummy = 0;
        double v = MODELS ? diag_model_value<T, false>(row, a.ML, a.D, a.dep, q, RANK_FINITE, dummy) : (double)row[q];
        v = v == 0.0 ? 0.0 : v;      // -0.0 is +0.0
        keys[pos] = okey_of((T)v);
        idx[pos] = elem;
    }
}

// the lanes of the wavefront whose digit equals this lane's (all lanes call it; the mask of an inactive lane means nothing)
__device__ __forceinline__ unsigned long long match_digit(unsigned d, bool active)
{
    unsigned long long m = __ballot(active);
#pragma unroll
    for (int b = 0; b < BH_RANK_RADIXBITS; ++b) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long v = __ballot(active && bit);
        m &= bit ? v : ~v;
    }
    return m;
}

// counts[tile][d]
template <typename K>
__global__ void __launch_bounds__(256) rank_hist_kernel(Pools p, const K *keys, int shift, unsigned *counts)
{
    __shared__ unsigned hist[256];
    const Tile t = tile_of(p, blockIdx.x);
    const int tid = threadIdx.x, lane = tid & 63;
    hist[tid] = 0;
    __syncthreads();
    for (unsigned base = t.lo; base < t.hi; base += 256) {      // (uniform: every lane takes every step)
        const unsigned pos = base + tid;
        const bool active = pos < t.hi;
        const unsigned d = active ? (unsigned)(keys[pos] >> shift) & 255u : 0u;
        const unsigned long long m = match_digit(d, active);
        if (active && (__ffsll((long long)m) - 1) == lane) atomicAdd(&hist[d], (unsigned)__popcll(m));
    }
    __syncthreads();
    counts[(size_t)blockIdx.x * 256 + tid] = hist[tid];
}

// counts[tile][d] -> the keys of digit d in the segment's tiles before this one; digit_base[g][d] = the segment's keys of smaller digits
__global__ void __launch_bounds__(256) rank_scan_kernel(Pools p, unsigned *counts, unsigned *digit_base)
{
    __shared__ unsigned tot[256];
    const int g = blockIdx.x, d = threadIdx.x;
    unsigned run = 0;
    for (int b = p.seg_blk0[g]; b < p.seg_blk0[g + 1]; ++b) {
        const unsigned c = counts[(size_t)b * 256 + d];
        counts[(size_t)b * 256 + d] = run;
        run += c;
    }
    tot[d] = run;
    __syncthreads();
    unsigned before = 0;
    for (int i = 0; i < d; ++i) before += tot[i];
    digit_base[(size_t)g * 256 + d] = before;
}

template <typename K>
__global__ void __launch_bounds__(256) rank_scatter_kernel(Pools p, const K *kin, const unsigned *iin, K *kout, unsigned *iout, int shift,
                                                           const unsigned *counts, const unsigned *digit_base)
{
    __shared__ unsigned base[256];
    __shared__ unsigned wc[4][256];
    const Tile t = tile_of(p, blockIdx.x);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    base[tid] = t.s0 + digit_base[(size_t)t.g * 256 + tid] + counts[(size_t)blockIdx.x * 256 + tid];
    wc[0][tid] = wc[1][tid] = wc[2][tid] = wc[3][tid] = 0;
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    for (unsigned b0 = t.lo; b0 < t.hi; b0 += 256) {
        const unsigned pos = b0 + tid;
        const bool active = pos < t.hi;
        const K k = active ? kin[pos] : (K)0;
        const unsigned id = active ? iin[pos] : 0u;
        const unsigned d = (unsigned)(k >> shift) & 255u;
        const unsigned long long m = match_digit(d, active);
        if (active && (__ffsll((long long)m) - 1) == lane) wc[w][d] = (unsigned)__popcll(m);
        __syncthreads();
        if (active) {
            unsigned off = base[d] + (unsigned)__popcll(m & below);
            for (int u = 0; u < w; ++u) off += wc[u][d];
            if (off >= t.s0 && off < t.s1) {      // (always, when hist and scatter saw the same keys)
                kout[off] = k;
                iout[off] = id;
            }
        }
        __syncthreads();
        base[tid] += wc[0][tid] + wc[1][tid] + wc[2][tid] + wc[3][tid];
        wc[0][tid] = wc[1][tid] = wc[2][tid] = wc[3][tid] = 0;
        __syncthreads();
    }
}

struct RankOut {
    double *z;       // z or zf (this launch)
    float *tail;     // with z only
    int64_t ld_t, ld_c;
    int q;           // the column of the outputs
    int C;
    const double *zt;
    const int64_t *zoff;
};

// the tie run of sorted position i: lt = its start, eq = its length, both relative to the segment
template <typename K>
__device__ __forceinline__ void tie_run(const K *s, unsigned n, unsigned i, unsigned &lt, unsigned &eq)
{
    const K k = s[i];
    unsigned lo = i, hi = i + 1;
    if (i > 0 && s[i - 1] == k) {          // the first j in [0, i) with s[j] == k (s[j] >= k)
        unsigned a = 0, b = i - 1;         // s[b] == k
        while (a < b) {
            const unsigned mid = a + (b - a) / 2;
            if (s[mid] < k) a = mid + 1; else b = mid;
        }
        lo = a;
    }
    if (i + 1 < n && s[i + 1] == k) {      // the first j in (i + 1, n] with j == n or s[j] > k
        unsigned a = i + 2, b = n;
        while (a < b) {
            const unsigned mid = a + (b - a) / 2;
            if (s[mid] > k) b = mid; else a = mid + 1;
        }
        hi = a;
    }
    lt = lo;
    eq = hi - lo;
}

template <typename K>
__global__ void __launch_bounds__(256) rank_write_kernel(Pools p, const K *keys, const unsigned *idx, RankOut o)
{
    const Tile t = tile_of(p, blockIdx.x);
    const unsigned n = t.s1 - t.s0;
    const double *zt = o.zt ? o.zt + o.zoff[t.g] : nullptr;
    const unsigned lo_max = (n - 1) / 20;
    const unsigned hi_max = (unsigned)((19ull * (unsigned long long)(n - 1)) / 20ull);
    for (unsigned pos = t.lo + threadIdx.x; pos < t.hi; pos += 256) {
        unsigned lt, eq;
        tie_run(keys + t.s0, n, pos - t.s0, lt, eq);
        const unsigned elem = idx[pos];
        const unsigned row = elem / (unsigned)o.C, c = elem - row * (unsigned)o.C;
        const int64_t at = (int64_t)row * o.ld_t + (int64_t)c * o.ld_c;
        if (o.z) o.z[at + o.q] = zt[2ull * lt + eq + 1ull];
        if (o.tail) {
            o.tail[2 * at + 2 * o.q] = lt <= lo_max ? 1.0f : 0.0f;
            o.tail[2 * at + 2 * o.q + 1] = lt <= hi_max ? 1.0f : 0.0f;
        }
    }
}

// the folded keys of a sorted segment, at the same positions (the element indices stay where they are)
template <typename K>
__global__ void __launch_bounds__(256) rank_fold_kernel(Pools p, const K *keys, unsigned long long *fkeys)
{
    const Tile t = tile_of(p, blockIdx.x);
    const unsigned n = t.s1 - t.s0;
    const double med = (okey_value(keys[t.s0 + (n - 1) / 2]) + okey_value(keys[t.s0 + n / 2])) * 0.5;
    for (unsigned pos = t.lo + threadIdx.x; pos < t.hi; pos += 256)
        fkeys[pos] = okey64(fabs(okey_value(keys[pos]) - med));
}

// 0 in every output of the chains left out: one thread per (row, such chain)
__global__ void __launch_bounds__(256) rank_zero_kernel(const int *left, int nleft, int64_t T, int Q, double *z, double *zf, float *tail,
                                                        int64_t ld_t, int64_t ld_c)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= T * nleft) return;
    const int64_t row = i / nleft;
    const int c = left[i - row * nleft];
    const int64_t at = row * ld_t + (int64_t)c * ld_c;
    for (int q = 0; q < Q; ++q) {
        if (z) z[at + q] = 0.0;
        if (zf) zf[at + q] = 0.0;
        if (tail) tail[2 * at + 2 * q] = tail[2 * at + 2 * q + 1] = 0.0f;
    }
}

// the scratch of one column and the sort of what lies in (k0, i0): `passes` stable passes, the result in (*kr, *ir)
struct Sorter {
    hipStream_t st;
    Pools p;
    unsigned tiles;
    int G;
    unsigned *counts, *digit_base;

    template <typename K> void run(K *k0, unsigned *i0, K *k1, unsigned *i1, K **kr, unsigned **ir) const
    {
        for (int pass = 0; pass < (int)sizeof(K); ++pass) {
            const int shift = BH_RANK_RADIXBITS * pass;
            rank_hist_kernel<K><<<dim3(tiles), 256, 0, st>>>(p, k0, shift, counts);
            rank_scan_kernel<<<dim3((unsigned)G), 256, 0, st>>>(p, counts, digit_base);
            rank_scatter_kernel<K><<<dim3(tiles), 256, 0, st>>>(p, k0, i0, k1, i1, shift, counts, digit_base);
            std::swap(k0, k1);
            std::swap(i0, i1);
        }
        *kr = k0;
        *ir = i0;
    }
};

template <typename T, bool MODELS>
int rank_all(bh_engine *e, hipStream_t st, const RankArgs &a, int q0, int nq, int Qcheck, unsigned tiles, int G, size_t M, bool host,
             const double *dzt, const int64_t *dzoff, const int *dleft, int nleft, double *z, double *zf, float *tail, int64_t ld_out_t,
             int64_t ld_out_c)
{
    typedef okey_t<T> K;
    int rc;
    Buf dflag, kA, kB, iA, iB, dcounts, ddigit, sz, szf, stail;
    if ((rc = alloc(e, dflag, 8))) return rc;
    BH_CHK(e, hipMemsetAsync(dflag.p, 0, 8, st));
    rank_check_kernel<T, MODELS><<<dim3(tiles), 256, 0, st>>>(a, Qcheck, dflag.as<int>());
    BH_CHK(e, hipGetLastError());
    int flag = 0;
    BH_CHK(e, hipMemcpyAsync(&flag, dflag.p, 4, hipMemcpyDeviceToHost, st));
    BH_CHK(e, hipStreamSynchronize(st));
    if (flag & 2) return fail(e, BH_EINVAL, "a model row's non-NaN values are not a non-empty prefix of even length");
    if (flag & 1) return fail(e, BH_EINVAL, "a value of a kept chain is not finite");
    if (!z && !zf && !tail) return BH_OK;

    if ((rc = alloc(e, kA, M * 8)) || (rc = alloc(e, kB, M * 8)) || (rc = alloc(e, iA, M * 4)) || (rc = alloc(e, iB, M * 4)) ||
        (rc = alloc(e, dcounts, (size_t)tiles * 256 * 4)) || (rc = alloc(e, ddigit, (size_t)G * 256 * 4)))
        return rc;
    // host outputs: one column at a time through [T][C] tables on the device (the chains left out stay 0 there)
    const size_t TC = (size_t)a.T * (size_t)a.C;
    std::vector<double> hz, hzf;
    std::vector<float> htail;
    RankOut o;
    o.C = a.C; o.zt = dzt; o.zoff = dzoff;
    if (host) {
        if (z) { if ((rc = alloc(e, sz, TC * 8))) return rc; BH_CHK(e, hipMemsetAsync(sz.p, 0, TC * 8, st)); hz.resize(TC); }
        if (zf) { if ((rc = alloc(e, szf, TC * 8))) return rc; BH_CHK(e, hipMemsetAsync(szf.p, 0, TC * 8, st)); hzf.resize(TC); }
        if (tail) { if ((rc = alloc(e, stail, TC * 8))) return rc; BH_CHK(e, hipMemsetAsync(stail.p, 0, TC * 8, st)); htail.resize(TC * 2); }
        o.ld_t = a.C; o.ld_c = 1;
    } else {
        o.ld_t = ld_out_t; o.ld_c = ld_out_c;
        if (nleft) {
            const int64_t n = a.T * nleft;
            rank_zero_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, st>>>(dleft, nleft, a.T, nq, z, zf, tail, ld_out_t, ld_out_c);
            BH_CHK(e, hipGetLastError());
        }
    }
    Sorter s;
    s.st = st; s.p = a.p; s.tiles = tiles; s.G = G; s.counts = dcounts.as<unsigned>(); s.digit_base = ddigit.as<unsigned>();
    for (int j = 0; j < nq; ++j) {
        rank_extract_kernel<T, MODELS><<<dim3(tiles), 256, 0, st>>>(a, q0 + j, kA.as<K>(), iA.as<unsigned>());
        K *ks;
        unsigned *is;
        s.run<K>(kA.as<K>(), iA.as<unsigned>(), kB.as<K>(), iB.as<unsigned>(), &ks, &is);
        if (z || tail) {
            o.z = host ? sz.as<double>() : z;
            o.tail = host ? stail.as<float>() : tail;
            if (!z) o.z = nullptr;
            if (!tail) o.tail = nullptr;
            o.q = host ? 0 : j;
            rank_write_kernel<K><<<dim3(tiles), 256, 0, st>>>(a.p, ks, is, o);
        }
        if (zf) {
            // the folded keys go to the key buffer the sorted keys are not in; the sorted indices start the second sort
            unsigned long long *f0 = (void *)ks == kA.p ? kB.as<unsigned long long>() : kA.as<unsigned long long>();
            unsigned long long *f1 = (void *)ks == kA.p ? kA.as<unsigned long long>() : kB.as<unsigned long long>();
            unsigned *j1 = is == iA.as<unsigned>() ? iB.as<unsigned>() : iA.as<unsigned>();
            rank_fold_kernel<K><<<dim3(tiles), 256, 0, st>>>(a.p, ks, f0);
            unsigned long long *fs;
            unsigned *js;
            s.run<unsigned long long>(f0, is, f1, j1, &fs, &js);
            o.z = host ? szf.as<double>() : zf;
            o.tail = nullptr;
            o.q = host ? 0 : j;
            rank_write_kernel<unsigned long long><<<dim3(tiles), 256, 0, st>>>(a.p, fs, js, o);
        }
        BH_CHK(e, hipGetLastError());
        if (host) {
            if (z) BH_CHK(e, hipMemcpyAsync(hz.data(), sz.p, TC * 8, hipMemcpyDeviceToHost, st));
            if (zf) BH_CHK(e, hipMemcpyAsync(hzf.data(), szf.p, TC * 8, hipMemcpyDeviceToHost, st));
            if (tail) BH_CHK(e, hipMemcpyAsync(htail.data(), stail.p, TC * 8, hipMemcpyDeviceToHost, st));
            BH_CHK(e, hipStreamSynchronize(st));
            for (int64_t t = 0; t < a.T; ++t)
                for (int c = 0; c < a.C; ++c) {
                    const size_t from = (size_t)t * (size_t)a.C + (size_t)c;
                    const int64_t at = t * ld_out_t + (int64_t)c * ld_out_c;
                    if (z) z[at + j] = hz[from];
                    if (zf) zf[at + j] = hzf[from];
                    if (tail) { tail[2 * at + 2 * j] = htail[2 * from]; tail[2 * at + 2 * j + 1] = htail[2 * from + 1]; }
                }
        }
    }
    BH_CHK(e, hipStreamSynchronize(st));
    return BH_OK;
}

int rank_run(bh_engine *e, bool models, int memspace, void *stream, int elem_bytes, int64_t T, int C, int Q, int ML, int D, int q0, int nq,
             int64_t ld_t, int64_t ld_c, const void *x, const double *dep, int G, const int32_t *group, const double *zt,
             const int64_t *zoff, double *z, double *zf, float *tail, int64_t ld_out_t, int64_t ld_out_c)
{
    int rc;
    bh_chain_refusal no;
    if (!e) return BH_EINVAL;
    if (elem_bytes != 4 && elem_bytes != 8) return fail(e, BH_EINVAL, "the table must be float32 or float64");
    if (!x || !group) return fail(e, BH_EINVAL, "null argument");
    if ((z || zf) && (!zt || !zoff)) return fail(e, BH_EINVAL, "z and zf need the table zt and its offsets zoff");
    if (models) {
        if ((no = bh_chain_model_table(ML, D, dep)).code) return fail(e, no.code, no.text);
        if (q0 < 0 || nq < 1 || q0 > D || nq > D + 1 - q0) return fail(e, BH_EINVAL, "columns: q0 .. q0 + nq - 1 within 0 .. D");
    } else {
        if (Q < 1 || Q > BH_DIAG_MAXCOLS) return fail(e, BH_EINVAL, "columns: 1..BH_DIAG_MAXCOLS per call");
        q0 = 0;
        nq = Q;
    }
    const int64_t width = models ? 2 * ML : Q;
    if ((no = bh_chain_table_span(T, C, width, ld_t, ld_c)).code) return fail(e, no.code, no.text);
    if ((long double)T * (long double)C >= 4294967296.0L) return fail(e, BH_EINVAL, "T * C must stay below 2^32");
    if ((z || zf || tail) &&
        (ld_out_t < 1 || ld_out_c < nq ||
         !((long double)(T - 1) * (long double)ld_out_t + (long double)(C - 1) * (long double)ld_out_c + (long double)nq < 5.76460752303423488e17L)))
        return fail(e, BH_EINVAL, "bad leading dimensions of the outputs");
    if (G < 1 || G > C) return fail(e, BH_EINVAL, "groups: 1 <= G <= C");
    std::vector<int> m((size_t)G, 0), left;
    for (int c = 0; c < C; ++c) {
        if (group[c] < -1 || group[c] >= G) return fail(e, BH_EINVAL, "a group value outside [-1, G)");
        if (group[c] < 0) left.push_back(c); else ++m[(size_t)group[c]];
    }
    std::vector<unsigned> seg_base((size_t)G + 1, 0u);
    std::vector<int> moff((size_t)G, 0), blk0((size_t)G + 1, 0), member((size_t)C - left.size()), blk_seg;
    std::vector<int64_t> hzoff((size_t)G, 0);
    size_t ztlen = 0;
    for (int g = 0; g < G; ++g) {
        if (!m[(size_t)g]) return fail(e, BH_EINVAL, "an empty group");
        const uint64_t N = (uint64_t)m[(size_t)g] * (uint64_t)T;
        if (z || zf) {
            if (zoff[g] < 0 || zoff[g] > ((int64_t)1 << 40)) return fail(e, BH_EINVAL, "a zoff that does not fit (0 .. 2^40)");
            hzoff[(size_t)g] = zoff[g];
            ztlen = std::max(ztlen, (size_t)zoff[g] + (size_t)(2 * N + 1));
        }
        moff[(size_t)g] = g ? moff[(size_t)g - 1] + m[(size_t)g - 1] : 0;
        seg_base[(size_t)g + 1] = seg_base[(size_t)g] + (unsigned)N;
        const int nb = (int)((N + RANK_TILE - 1) / RANK_TILE);
        blk0[(size_t)g + 1] = blk0[(size_t)g] + nb;
        blk_seg.insert(blk_seg.end(), (size_t)nb, g);
    }
    {
        std::vector<int> fill(moff);
        for (int c = 0; c < C; ++c)
            if (group[c] >= 0) member[(size_t)fill[(size_t)group[c]]++] = c;
    }
    const size_t M = seg_base[(size_t)G];
    const unsigned tiles = (unsigned)blk_seg.size();

    BH_CHK(e, hipSetDevice(bh_engine_device_internal(e)));
    const bool host = memspace != BH_DEVICE;
    hipStream_t st = call_stream(e, memspace, stream);
    Buf copy, ddep, dbase, dm, dmoff, dblk0, dmember, dblkseg, dleft, dzt, dzoff;
    RankArgs a;
    const size_t span = (size_t)((T - 1) * ld_t + (int64_t)(C - 1) * ld_c + width) * (size_t)elem_bytes;
    if ((rc = stage(e, st, memspace, x, span, copy, &a.x))) return rc;
    a.T = T; a.ld_t = ld_t; a.ld_c = ld_c; a.C = C; a.ML = ML; a.D = D; a.dep = nullptr;
    if (models && D) {
        if ((rc = alloc(e, ddep, (size_t)D * 8))) return rc;
        BH_CHK(e, hipMemcpyAsync(ddep.p, dep, (size_t)D * 8, hipMemcpyHostToDevice, st));
        a.dep = ddep.as<double>();
    }
    if ((rc = upload(e, st, dbase, seg_base)) || (rc = upload(e, st, dm, m)) || (rc = upload(e, st, dmoff, moff)) ||
        (rc = upload(e, st, dblk0, blk0)) || (rc = upload(e, st, dmember, member)) || (rc = upload(e, st, dblkseg, blk_seg)) ||
        (rc = upload(e, st, dleft, left)) || (rc = upload(e, st, dzoff, hzoff)))
        return rc;
    if (z || zf) {
        if ((rc = alloc(e, dzt, ztlen * 8))) return rc;
        BH_CHK(e, hipMemcpyAsync(dzt.p, zt, ztlen * 8, hipMemcpyHostToDevice, st));
    }
    a.p.seg_base = dbase.as<unsigned>(); a.p.seg_m = dm.as<int>(); a.p.seg_moff = dmoff.as<int>(); a.p.seg_blk0 = dblk0.as<int>();
    a.p.member = dmember.as<int>(); a.p.blk_seg = dblkseg.as<int>();
    const double *pzt = (z || zf) ? dzt.as<double>() : nullptr;
#define RANK_GO(TT, MM)                                                                                                           \
    rank_all<TT, MM>(e, st, a, q0, nq, Q, tiles, G, M, host, pzt, dzoff.as<int64_t>(), dleft.as<int>(), (int)left.size(), z, zf, tail, \
                     ld_out_t, ld_out_c)
    if (models) rc = elem_bytes == 4 ? RANK_GO(float, true) : RANK_GO(double, true);
    else rc = elem_bytes == 4 ? RANK_GO(float, false) : RANK_GO(double, false);
#undef RANK_GO
    (void)hipStreamSynchronize(st);   // (the buffers and the host vectors go with this frame)
    return rc;
}

} // namespace

extern "C" {

int bh_chain_rank_series(bh_engine *e, int memspace, void *stream, int elem_bytes, int64_t T, int C, int Q, int64_t ld_t,
                         int64_t ld_c, const void *x, int G, const int32_t *group, const double *zt, const int64_t *zoff,
                         double *z, double *zf, float *tail, int64_t ld_out_t, int64_t ld_out_c)
{
    return rank_run(e, false, memspace, stream, elem_bytes, T, C, Q, 0, 0, 0, Q, ld_t, ld_c, x, nullptr, G, group, zt, zoff, z, zf, tail,
                    ld_out_t, ld_out_c);
}

int bh_chain_rank_models(bh_engine *e, int memspace, void *stream, int elem_bytes, int64_t T, int C, int ML, int64_t ld_t,
                         int64_t ld_c, const void *models, int D, const double *dep, int q0, int nq, int G, const int32_t *group,
                         const double *zt, const int64_t *zoff, double *z, double *zf, float *tail, int64_t ld_out_t,
                         int64_t ld_out_c)
{
    return rank_run(e, true, memspace, stream, elem_bytes, T, C, 0, ML, D, q0, nq, ld_t, ld_c, models, dep, G, group, zt, zoff, z, zf,
                    tail, ld_out_t, ld_out_c);
}

} // extern "C"
