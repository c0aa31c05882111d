// bayhunter_amd/csrc/chain_diag_kernel.hip -- order statistics of the chains' recorded series (include/bh_engine_chain_diag.h).
//
// The tables are read where record="device" wrote them, [rows][C][Q]: a series is one (chain, column), its samples ld_t apart.
// Nothing is transposed or copied; a value of a model table (the vs at a depth, the number of layers) is formed from its row
// where it is needed.
//
// sum kernel : one workgroup per chain.  Thread (column q, strand s) adds the samples i = s (mod 16) of its column in ascending i
//              into the accumulators of the two halves, a fixed tree combines the 16 strands.  Consecutive threads read consecutive
//              columns of one row.  Mode 0: x0, S1, S1a, S1b, and the check of every value; mode 1, with the means the host formed
//              in between: M2a, M2b.
// lag kernel : one workgroup per (chain, column, block of BH_DIAG_LAGBLOCK lags).  It walks the series in tiles of BH_DIAG_TILE
//              rows: e_i of the tile in LDS (2 KB), and behind it a ring of 2048 e's (16 KB) that holds the halo e_{i+k} of the
//              block's lags -- every sample is read from memory once per workgroup.  Thread t owns the lags kb + t + 256 j, j < 4,
//              in four FP64 registers and adds e_i * e_{i+k} in ascending i: e_i is one LDS address for the whole wavefront (a
//              broadcast), e_{i+k} consecutive addresses in consecutive lanes (ds_read_b64, 32 lanes = one 256-B bank row: no
//              conflict).  Rows at and beyond T are zeros in LDS: their products add +-0 to a sum that is never -0, so the bits
//              are those of the sum over i < T-k.
// medians    : one workgroup per chain, a radix selection (8 bits per pass, 256 LDS counters) on the ordered bit patterns.
// gathered   : the same kernel bodies for series that read another chain at every row (include/bh_engine_chain_diag_ladders.h):
//              series k reads chain sel[t][k], one int load per value; the index is clamped before it addresses anything and a
//              clamped one is flagged by the first pass.  Strands, tree and ring are the bodies' own, so the bits are those of the
//              table gathered on the host.  The builds without a selection are the bodies with the chain fixed: as before.
// -ffp-contract=off (Makefile): no product is contracted into a sum; that is part of the contract of the header.
#include "bh_hostkit.h"
#include "bh_okey.h"
#include "chain_diag_value.h"
#include "chain_tables.h"
#include "../../include/bh_engine_chain_diag.h"
#include "../../include/bh_engine_chain_diag_ladders.h"

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#pragma clang fp contract(off)

#define DIAG_RING 2048
#define DIAG_BIG 0x1p480     // a value beyond it (or not finite) is refused: e_i * e_j and their sums then stay finite

static_assert(BH_DIAG_LAGBLOCK + 3 * BH_DIAG_TILE <= DIAG_RING, "ring: the live rows of two neighbouring tiles and the rows being loaded");
static_assert(BH_DIAG_LAGBLOCK == 4 * 256 && BH_DIAG_TILE == 256 && BH_DIAG_STRANDS == 16, "thread layout of the kernels");

namespace {

using namespace bhkit;

struct DiagArgs {
    const void *x;
    int64_t T, ld_t, ld_c;
    int Q, L, ML, D;
    const double *dep;   // device [D] (models)
};

// ... and of gathered series: series k reads chain sel[t*ld_sel + k] of the C chains at row t
struct DiagSelArgs : DiagArgs {
    const int32_t *sel;
    int64_t ld_sel;
    int C;
};

// the chain that series c reads at row t: c itself, or the selected one -- clamped into [0, C) before it is an address, flagged
template <bool CHECK> __device__ __forceinline__ int chain_at(const DiagArgs &, int c, int64_t, int &) { return c; }
template <bool CHECK> __device__ __forceinline__ int chain_at(const DiagSelArgs &a, int k, int64_t t, int &bad)
{
    const int c = a.sel[t * a.ld_sel + k];
    const int cc = min(max(c, 0), a.C - 1);
    if (CHECK && cc != c) bad |= 4;
    return cc;
}

// the value (t, c, q) of a table of series ...
template <typename T, bool MODELS, bool CHECK, typename Args>
__device__ __forceinline__ double value(const Args &a, int c, int64_t t, int q, int &bad)
{
    const T *row = (const T *)a.x + t * a.ld_t + (int64_t)chain_at<CHECK>(a, c, t, bad) * a.ld_c;
    if (!MODELS) {
        const double v = (double)row[q];
        if (CHECK && !(fabs(v) <= DIAG_BIG)) bad |= 1;
        return v;
    }
    // ... and of a table of model rows [vs_1..vs_n, z_1..z_n, NaN...]: vs[#{j : d_j <= dep[q]}] (the rule of bh_engine_posterior.h,
    // posterior_kernel.hip), column D: n - 1 -- chain_diag_value.h, shared with the rank transform
    return diag_model_value<T, CHECK>(row, a.ML, a.D, a.dep, q, DIAG_BIG, bad);
}

__device__ __forceinline__ double strand_tree(const double (*p)[BH_DIAG_MAXCOLS], int q)
{
    return (((p[0][q] + p[1][q]) + (p[2][q] + p[3][q])) + ((p[4][q] + p[5][q]) + (p[6][q] + p[7][q]))) +
           (((p[8][q] + p[9][q]) + (p[10][q] + p[11][q])) + ((p[12][q] + p[13][q]) + (p[14][q] + p[15][q])));
}

// MODE 0: out[c][q][4] = x0, S1, S1a, S1b;  MODE 1: out[c][q][2] = M2a, M2b with means[c][q][3] = m, ma, mb
template <typename T, bool MODELS, int MODE, typename Args>
__device__ __forceinline__ void diag_sum_body(const Args a, const double *means, double *out, int *flag)
{
    __shared__ double part[3][BH_DIAG_STRANDS][BH_DIAG_MAXCOLS];
    const int c = blockIdx.x, Q = a.Q;
    const int64_t Tn = a.T, h = Tn / 2;
    int bad = 0;
    for (int w = threadIdx.x; w < Q * BH_DIAG_STRANDS; w += 256) {
        const int q = w % Q, s = w / Q;
        const double x0 = value<T, MODELS, MODE == 0>(a, c, 0, q, bad);
        const double ma = MODE ? means[((size_t)c * Q + q) * 3 + 1] : 0.0, mb = MODE ? means[((size_t)c * Q + q) * 3 + 2] : 0.0;
        double A = 0.0, B = 0.0, M = 0.0;
        for (int64_t i = s; i < Tn; i += BH_DIAG_STRANDS) {
            const double d = value<T, MODELS, MODE == 0>(a, c, i, q, bad) - x0;
            if (MODE == 0 && !(fabs(d) <= DIAG_BIG)) bad |= 1;
            if (i < h) {
                const double u = d - ma;
                A += MODE ? u * u : d;
            } else if (i >= Tn - h) {
                const double u = d - mb;
                B += MODE ? u * u : d;
            } else {
                M = d;
            }
        }
        part[0][s][q] = A;
        part[1][s][q] = B;
        part[2][s][q] = M;
    }
    __syncthreads();
    if ((int)threadIdx.x < Q) {
        const int q = threadIdx.x;
        const double A = strand_tree(part[0], q), B = strand_tree(part[1], q);
        if (MODE == 0) {
            double *o = out + ((size_t)c * Q + q) * 4;
            int dummy = 0;
            o[0] = value<T, MODELS, false>(a, c, 0, q, dummy);
            o[1] = (Tn & 1) ? (A + part[2][h % BH_DIAG_STRANDS][q]) + B : A + B;
            o[2] = A;
            o[3] = B;
        } else {
            double *o = out + ((size_t)c * Q + q) * 2;
            o[0] = A;
            o[1] = B;
        }
    }
    if (MODE == 0 && bad) atomicOr(flag, bad);
}

template <typename T, bool MODELS, int MODE, typename Args>
__global__ void __launch_bounds__(256) diag_sum_kernel(Args a, const double *means, double *out, int *flag)
{
    diag_sum_body<T, MODELS, MODE>(a, means, out, flag);
}

// P[c][q][k], k = kb .. min(kb + BH_DIAG_LAGBLOCK - 1, L), kb = blockIdx.z * BH_DIAG_LAGBLOCK
template <typename T, bool MODELS, typename Args>
__device__ __forceinline__ void diag_lag_body(const Args a, const double *means, double *P)
{
    __shared__ double ea[BH_DIAG_TILE];
    __shared__ double ring[DIAG_RING];
    const int c = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
    const int kb = blockIdx.z * BH_DIAG_LAGBLOCK;
    const int nl = min(BH_DIAG_LAGBLOCK, a.L + 1 - kb);   // the block's lags
    const int nj = (nl + 255) / 256;
    const int64_t Tn = a.T;
    int dummy = 0;
    const double x0 = value<T, MODELS, false>(a, c, 0, q, dummy);
    const double m = means[((size_t)c * a.Q + q) * 3];
    // rows [kb, kb + LAGBLOCK) of the ring; every tile then brings the TILE rows behind its halo
    for (int r = tid; r < BH_DIAG_LAGBLOCK; r += 256) {
        const int64_t j = (int64_t)kb + r;
        ring[j & (DIAG_RING - 1)] = j < Tn ? (value<T, MODELS, false>(a, c, j, q, dummy) - x0) - m : 0.0;
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t t0 = 0; t0 < Tn - kb; t0 += BH_DIAG_TILE) {
        const int64_t i = t0 + tid, j = t0 + kb + BH_DIAG_LAGBLOCK + tid;
        const double ei = i < Tn ? (value<T, MODELS, false>(a, c, i, q, dummy) - x0) - m : 0.0;
        const double ej = j < Tn ? (value<T, MODELS, false>(a, c, j, q, dummy) - x0) - m : 0.0;
        __syncthreads();   // the tile before is done with ea
        ea[tid] = ei;
        ring[j & (DIAG_RING - 1)] = ej;
        __syncthreads();
        const int base = (int)((t0 + kb) & (DIAG_RING - 1)) + tid;
#pragma unroll 4
        for (int ii = 0; ii < BH_DIAG_TILE; ++ii) {
            const double av = ea[ii];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
                if (jj < nj) acc[jj] += av * ring[(base + ii + 256 * jj) & (DIAG_RING - 1)];
        }
    }
    double *o = P + ((size_t)c * a.Q + q) * (size_t)(a.L + 1);
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const int k = kb + tid + 256 * jj;
        if (k <= a.L) o[k] = acc[jj];
    }
}

template <typename T, bool MODELS, typename Args>
__global__ void __launch_bounds__(256) diag_lag_kernel(Args a, const double *means, double *P)
{
    diag_lag_body<T, MODELS>(a, means, P);
}

// out[c][2]: the values of ranks (T-1)/2 and T/2 of chain c's column
template <typename T, typename Args>
__device__ __forceinline__ void diag_median_body(const Args a, double *out, int *flag)
{
    typedef okey_t<T> K;
    __shared__ unsigned hist[256];
    __shared__ K s_prefix;
    __shared__ unsigned long long s_rank;
    const int c = blockIdx.x, tid = threadIdx.x;
    const int64_t Tn = a.T;
    const T *x = (const T *)a.x;
    int bad = 0;
    for (int r = 0; r < 2; ++r) {
        if (tid == 0) {
            s_prefix = 0;
            s_rank = (unsigned long long)(r ? Tn / 2 : (Tn - 1) / 2);
        }
        for (int pass = (int)sizeof(T) - 1; pass >= 0; --pass) {
            const int shift = 8 * pass;
            hist[tid] = 0;
            __syncthreads();
            const K prefix = s_prefix;
            const K himask = pass == (int)sizeof(T) - 1 ? (K)0 : (K)(~(K)0 << (shift + 8));
            for (int64_t i = tid; i < Tn; i += 256) {
                const T v = x[i * a.ld_t + (int64_t)chain_at<true>(a, c, i, bad) * a.ld_c];
                if (r == 0 && pass == (int)sizeof(T) - 1 && !(fabs((double)v) <= 1.7976931348623157e308)) bad |= 1;
                const K k = okey_of(v);
                if ((k & himask) == prefix) atomicAdd(&hist[(unsigned)(k >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                unsigned long long rank = s_rank, cum = 0;
                int d = 0;
                for (; d < 255; ++d) {
                    if (cum + hist[d] > rank) break;
                    cum += hist[d];
                }
                s_prefix = prefix | ((K)d << shift);
                s_rank = rank - cum;
            }
            __syncthreads();
        }
        if (tid == 0) out[2 * (size_t)c + r] = okey_value(s_prefix);
        __syncthreads();
    }
    if (bad) atomicOr(flag, bad);
}

template <typename T, typename Args>
__global__ void __launch_bounds__(256) diag_median_kernel(Args a, double *out, int *flag)
{
    diag_median_body<T>(a, out, flag);
}

// the bytes a host table and a host selection cover (checked: bh_chain_table_span, bh_chain_sel_span)
size_t table_bytes(int elem_bytes, int64_t T, int C, int64_t width, int64_t ld_t, int64_t ld_c)
{
    return (size_t)((T - 1) * ld_t + (int64_t)(C - 1) * ld_c + width) * (size_t)elem_bytes;
}
size_t sel_bytes(int64_t T, int K, int64_t ld_sel) { return (size_t)((T - 1) * ld_sel + K) * sizeof(int32_t); }

// the kernels of a call: without a selection (Args = DiagArgs) and gathered (DiagSelArgs)
template <typename T, bool MODELS, int MODE, typename Args>
void launch_sum(hipStream_t st, unsigned n, const Args &a, const double *means, double *out, int *flag)
{
    diag_sum_kernel<T, MODELS, MODE, Args><<<dim3(n), 256, 0, st>>>(a, means, out, flag);
}
template <typename T, bool MODELS, typename Args> void launch_lag(hipStream_t st, dim3 grid, const Args &a, const double *means, double *P)
{
    diag_lag_kernel<T, MODELS, Args><<<grid, 256, 0, st>>>(a, means, P);
}
template <typename T, typename Args> void launch_median(hipStream_t st, unsigned n, const Args &a, double *out, int *flag)
{
    diag_median_kernel<T, Args><<<dim3(n), 256, 0, st>>>(a, out, flag);
}

// C: the series of the call (the chains, or the gathered series)
template <typename T, bool MODELS, typename Args>
int launch_all(bh_engine *e, hipStream_t st, const Args &a, int C, double *x0, double *s1, double *s1a, double *s1b, double *m2a,
               double *m2b, double *p)
{
    int rc;
    const size_t nser = (size_t)C * a.Q, np = nser * (size_t)(a.L + 1);
    Buf dsum, dmean, dm2, dP, dflag;
    if ((rc = alloc(e, dsum, nser * 32)) || (rc = alloc(e, dmean, nser * 24)) || (rc = alloc(e, dm2, nser * 16)) ||
        (rc = alloc(e, dP, np * 8)) || (rc = alloc(e, dflag, 8)))
        return rc;
    BH_CHK(e, hipMemsetAsync(dflag.p, 0, 8, st));
    launch_sum<T, MODELS, 0>(st, (unsigned)C, a, nullptr, dsum.as<double>(), dflag.as<int>());
    BH_CHK(e, hipGetLastError());
    std::vector<double> hs(nser * 4), hm(nser * 3), h2(nser * 2);
    int flag = 0;
    BH_CHK(e, hipMemcpyAsync(hs.data(), dsum.p, nser * 32, hipMemcpyDeviceToHost, st));
    BH_CHK(e, hipMemcpyAsync(&flag, dflag.p, 4, hipMemcpyDeviceToHost, st));
    BH_CHK(e, hipStreamSynchronize(st));
    if (flag & 4) return fail(e, BH_EINVAL, "a selection index is outside [0, C)");
    if (flag & 2) return fail(e, BH_EINVAL, "a model row's non-NaN values are not a non-empty prefix of even length");
    if (flag & 1) return fail(e, BH_EINVAL, "a value is not finite (or beyond 2^480)");
    const int64_t h = a.T / 2;
    for (size_t i = 0; i < nser; ++i) {
        hm[3 * i] = hs[4 * i + 1] / (double)a.T;
        hm[3 * i + 1] = h ? hs[4 * i + 2] / (double)h : 0.0;
        hm[3 * i + 2] = h ? hs[4 * i + 3] / (double)h : 0.0;
    }
    BH_CHK(e, hipMemcpyAsync(dmean.p, hm.data(), nser * 24, hipMemcpyHostToDevice, st));
    launch_sum<T, MODELS, 1>(st, (unsigned)C, a, dmean.as<double>(), dm2.as<double>(), nullptr);
    BH_CHK(e, hipGetLastError());
    const unsigned nblk = (unsigned)(a.L / BH_DIAG_LAGBLOCK + 1);
    launch_lag<T, MODELS>(st, dim3((unsigned)C, (unsigned)a.Q, nblk), a, dmean.as<double>(), dP.as<double>());
    BH_CHK(e, hipGetLastError());
    BH_CHK(e, hipMemcpyAsync(h2.data(), dm2.p, nser * 16, hipMemcpyDeviceToHost, st));
    BH_CHK(e, hipMemcpyAsync(p, dP.p, np * 8, hipMemcpyDeviceToHost, st));
    BH_CHK(e, hipStreamSynchronize(st));
    for (size_t i = 0; i < nser; ++i) {
        x0[i] = hs[4 * i];
        s1[i] = hs[4 * i + 1];
        s1a[i] = hs[4 * i + 2];
        s1b[i] = hs[4 * i + 3];
        m2a[i] = h2[2 * i];
        m2b[i] = h2[2 * i + 1];
    }
    return BH_OK;
}

template <typename Args>
int launch_typed(bh_engine *e, hipStream_t st, bool models, int elem_bytes, const Args &a, int nser, double *x0, double *s1, double *s1a,
                 double *s1b, double *m2a, double *m2b, double *p)
{
    if (models)
        return elem_bytes == 4 ? launch_all<float, true>(e, st, a, nser, x0, s1, s1a, s1b, m2a, m2b, p)
                               : launch_all<double, true>(e, st, a, nser, x0, s1, s1a, s1b, m2a, m2b, p);
    return elem_bytes == 4 ? launch_all<float, false>(e, st, a, nser, x0, s1, s1a, s1b, m2a, m2b, p)
                           : launch_all<double, false>(e, st, a, nser, x0, s1, s1a, s1b, m2a, m2b, p);
}

// gathered: K series that read chain sel[t*ld_sel + k] at row t (include/bh_engine_chain_diag_ladders.h); else sel is not looked at
int diag_run(bh_engine *e, bool models, int memspace, void *stream, int elem_bytes, int64_t T, int C, int Q, int ML, int D,
             int64_t ld_t, int64_t ld_c, const void *x, const double *dep, int L, double *x0, double *s1, double *s1a, double *s1b,
             double *m2a, double *m2b, double *p, bool gathered = false, int K = 0, const int32_t *sel = nullptr, int64_t ld_sel = 0)
{
    int rc;
    bh_chain_refusal no;
    if (!e) return BH_EINVAL;
    if (elem_bytes != 4 && elem_bytes != 8) return fail(e, BH_EINVAL, "the table must be float32 or float64");
    if (!x || !x0 || !s1 || !s1a || !s1b || !m2a || !m2b || !p) return fail(e, BH_EINVAL, "null argument");
    if (L < 0 || L > BH_DIAG_MAXLAG) return fail(e, BH_EINVAL, "maxlag must be 0..BH_DIAG_MAXLAG");
    if (models) {
        if ((no = bh_chain_model_table(ML, D, dep)).code) return fail(e, no.code, no.text);
        Q = D + 1;
    } else if (Q < 1 || Q > BH_DIAG_MAXCOLS) {
        return fail(e, BH_EINVAL, "columns: 1..BH_DIAG_MAXCOLS per call");
    }
    const int64_t width = models ? 2 * ML : Q;
    if ((no = bh_chain_table_span(T, C, width, ld_t, ld_c)).code) return fail(e, no.code, no.text);
    if (gathered && (no = bh_chain_sel_span(T, K, sel != nullptr, ld_sel)).code) return fail(e, no.code, no.text);
    BH_CHK(e, hipSetDevice(bh_engine_device_internal(e)));
    hipStream_t st = call_stream(e, memspace, stream);
    Buf copy, ddep, csel;
    DiagSelArgs a;
    a.sel = nullptr; a.ld_sel = ld_sel; a.C = C;
    if ((rc = stage(e, st, memspace, x, table_bytes(elem_bytes, T, C, width, ld_t, ld_c), copy, &a.x))) return rc;
    if (gathered && (rc = stage(e, st, memspace, sel, sel_bytes(T, K, ld_sel), csel, &a.sel))) return rc;
    a.T = T; a.ld_t = ld_t; a.ld_c = ld_c; a.Q = Q; a.L = L; a.ML = ML; a.D = D; a.dep = nullptr;
    if (models && D) {
        if ((rc = alloc(e, ddep, (size_t)D * 8))) return rc;
        BH_CHK(e, hipMemcpyAsync(ddep.p, dep, (size_t)D * 8, hipMemcpyHostToDevice, st));
        a.dep = ddep.as<double>();
    }
    rc = gathered ? launch_typed(e, st, models, elem_bytes, a, K, x0, s1, s1a, s1b, m2a, m2b, p)
                  : launch_typed(e, st, models, elem_bytes, (const DiagArgs &)a, C, x0, s1, s1a, s1b, m2a, m2b, p);
    if (rc != BH_OK) (void)hipStreamSynchronize(st);   // (the buffers go with this frame)
    return rc;
}

} // namespace

extern "C" {

int bh_chain_diag_series(bh_engine *e, int memspace, void *stream, int elem_bytes, int64_t T, int C, int Q, int64_t ld_t,
                         int64_t ld_c, const void *x, int L, double *x0, double *s1, double *s1a, double *s1b, double *m2a,
                         double *m2b, double *p)
{
    return diag_run(e, false, memspace, stream, elem_bytes, T, C, Q, 0, 0, ld_t, ld_c, x, nullptr, L, x0, s1, s1a, s1b, m2a, m2b, p);
}

int bh_chain_diag_models(bh_engine *e, int memspace, void *stream, int elem_bytes, int64_t T, int C, int ML, int64_t ld_t,
                         int64_t ld_c, const void *models, int D, const double *dep, int L, double *x0, double *s1, double *s1a,
                         double *s1b, double *m2a, double *m2b, double *p)
{
    return diag_run(e, true, memspace, stream, elem_bytes, T, C, 0, ML, D, ld_t, ld_c, models, dep, L, x0, s1, s1a, s1b, m2a, m2b, p);
}

} // extern "C"

namespace {

int median_run(bh_engine *e, int memspace, void *stream, int elem_bytes, int64_t T, int C, int64_t ld_t, int64_t ld_c, const void *x,
               double *lo, double *hi, bool gathered, int K, const int32_t *sel, int64_t ld_sel)
{
    int rc;
    bh_chain_refusal no;
    if (!e) return BH_EINVAL;
    if (elem_bytes != 4 && elem_bytes != 8) return fail(e, BH_EINVAL, "the table must be float32 or float64");
    if (!x || !lo || !hi) return fail(e, BH_EINVAL, "null argument");
    if ((no = bh_chain_table_span(T, C, 1, ld_t, ld_c)).code) return fail(e, no.code, no.text);
    if (T >= ((int64_t)1 << 32)) return fail(e, BH_EINVAL, "bad T, C or leading dimensions");   // (the ranks are 32-bit counts)
    if (gathered && (no = bh_chain_sel_span(T, K, sel != nullptr, ld_sel)).code) return fail(e, no.code, no.text);
    BH_CHK(e, hipSetDevice(bh_engine_device_internal(e)));
    hipStream_t st = call_stream(e, memspace, stream);
    Buf copy, dout, dflag, csel;
    DiagSelArgs a;
    a.sel = nullptr; a.ld_sel = ld_sel; a.C = C;
    if ((rc = stage(e, st, memspace, x, table_bytes(elem_bytes, T, C, 1, ld_t, ld_c), copy, &a.x))) return rc;
    if (gathered && (rc = stage(e, st, memspace, sel, sel_bytes(T, K, ld_sel), csel, &a.sel))) return rc;
    a.T = T; a.ld_t = ld_t; a.ld_c = ld_c; a.Q = 1; a.L = 0; a.ML = 0; a.D = 0; a.dep = nullptr;
    const int nser = gathered ? K : C;
    if ((rc = alloc(e, dout, (size_t)nser * 16)) || (rc = alloc(e, dflag, 8))) return rc;
    BH_CHK(e, hipMemsetAsync(dflag.p, 0, 8, st));
    if (gathered) {
        if (elem_bytes == 4) launch_median<float>(st, (unsigned)nser, a, dout.as<double>(), dflag.as<int>());
        else launch_median<double>(st, (unsigned)nser, a, dout.as<double>(), dflag.as<int>());
    } else {
        if (elem_bytes == 4) launch_median<float>(st, (unsigned)nser, (const DiagArgs &)a, dout.as<double>(), dflag.as<int>());
        else launch_median<double>(st, (unsigned)nser, (const DiagArgs &)a, dout.as<double>(), dflag.as<int>());
    }
    BH_CHK(e, hipGetLastError());
    std::vector<double> ho((size_t)nser * 2);
    int flag = 0;
    BH_CHK(e, hipMemcpyAsync(ho.data(), dout.p, (size_t)nser * 16, hipMemcpyDeviceToHost, st));
    BH_CHK(e, hipMemcpyAsync(&flag, dflag.p, 4, hipMemcpyDeviceToHost, st));
    BH_CHK(e, hipStreamSynchronize(st));
    if (flag & 4) return fail(e, BH_EINVAL, "a selection index is outside [0, C)");
    if (flag) return fail(e, BH_EINVAL, "a value is not finite");
    for (int c = 0; c < nser; ++c) {
        lo[c] = ho[2 * (size_t)c];
        hi[c] = ho[2 * (size_t)c + 1];
    }
    return BH_OK;
}

} // namespace

extern "C" {

int bh_chain_diag_medians(bh_engine *e, int memspace, void *stream, int elem_bytes, int64_t T, int C, int64_t ld_t, int64_t ld_c,
                          const void *x, double *lo, double *hi)
{
    return median_run(e, memspace, stream, elem_bytes, T, C, ld_t, ld_c, x, lo, hi, false, 0, nullptr, 0);
}

int bh_chain_diag_series_sel(bh_engine *e, int memspace, void *stream, int elem_bytes, int64_t T, int C, int Q, int64_t ld_t,
                             int64_t ld_c, const void *x, int K, const int32_t *sel, int64_t ld_sel, int L, double *x0, double *s1,
                             double *s1a, double *s1b, double *m2a, double *m2b, double *p)
{
    return diag_run(e, false, memspace, stream, elem_bytes, T, C, Q, 0, 0, ld_t, ld_c, x, nullptr, L, x0, s1, s1a, s1b, m2a, m2b, p,
                    true, K, sel, ld_sel);
}

int bh_chain_diag_models_sel(bh_engine *e, int memspace, void *stream, int elem_bytes, int64_t T, int C, int ML, int64_t ld_t,
                             int64_t ld_c, const void *models, int K, const int32_t *sel, int64_t ld_sel, int D, const double *dep,
                             int L, double *x0, double *s1, double *s1a, double *s1b, double *m2a, double *m2b, double *p)
{
    return diag_run(e, true, memspace, stream, elem_bytes, T, C, 0, ML, D, ld_t, ld_c, models, dep, L, x0, s1, s1a, s1b, m2a, m2b, p,
                    true, K, sel, ld_sel);
}

int bh_chain_diag_medians_sel(bh_engine *e, int memspace, void *stream, int elem_bytes, int64_t T, int C, int64_t ld_t,
                              int64_t ld_c, const void *x, int K, const int32_t *sel, int64_t ld_sel, double *lo, double *hi)
{
    return median_run(e, memspace, stream, elem_bytes, T, C, ld_t, ld_c, x, lo, hi, true, K, sel, ld_sel);
}

} // extern "C"
