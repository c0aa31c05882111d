// bayhunter_amd/csrc/chain_ladder_evidence_kernel.hip -- the rung series of tempered runs and the sums of their evidence estimates:
// bh_chain_ladder_holders, bh_chain_ladder_evidence (include/bh_engine_chain_ladder_evidence.h).
//
// The tables are read where record="device" wrote them, [rows][chains]: nothing is sorted, gathered or transposed.
//
// holder kernel   : the rung comparison of chain_ladder_kernel.hip, one thread per (t, c), consecutive threads consecutive chains of
//                   one row.  rung = the number of larger betas among the ladder's members; the thread at rung r writes
//                   hold[t][start[k] + r] = c -- one writer per element, no atomics.  It also counts the equal betas: a second one
//                   is a tie (two holders of one rung), flagged with a beta that is not finite.  hold is the call's own table; the
//                   caller's is filled from it by a kernel that first looks at the flags, so that a refusal writes nothing.
// extremes kernel : lanes along the series j of one row, rows over the wavefronts and the workgroups of a column of the grid.  Per
//                   series the largest and the smallest like (exact: no order), the finiteness of the likes, and the bits of the
//                   beta its holder has against row 0's.  A second small kernel combines the workgroups' partials and forms the
//                   steps of beta: the sum kernel's parameters never visit the host.
// sum kernel      : one workgroup = 8 series x 2 directions x the 16 strands: lanes along the series j of one row (the dependent reads
//                   x[t][hold] stay inside a ladder's own neighbouring elements), the forward and the reverse sum of a series in two
//                   lanes that read the same addresses, four strands -- four neighbouring rows -- per wavefront.  The order of the
//                   strands caps the parallelism at 32 threads per series, so each thread keeps eight rows in flight: the loads,
//                   then eight independent exp, then the additions in ascending t.  The strands are combined in the tree of
//                   chain_diag_kernel.hip.  exp is bh_libm.h's restatement of glibc's, its table staged in LDS once per workgroup; a
//                   term at or below -512 is 0 by selection: the device library's exp is never called.
// One stream synchronisation per BH_DEVICE call: the flags of both checking passes are read with the results.
// -ffp-contract=off (Makefile): the FMAs of bh_libm.h are explicit, and no product is contracted into a sum.
#include "bh_hostkit.h"
#include "chain_tables.h"
#define BH_HD __device__ __forceinline__
#define BH_TAB static __device__ const
#include "bh_libm.h"
#include "../../include/bh_engine_chain_ladder_evidence.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#pragma clang fp contract(off)

#define EV_SERIES 8      // series of one workgroup of the sum kernel
#define EV_FLIGHT 8      // rows a thread of the sum kernel has in flight
#define EV_ROWBLOCKS 64  // workgroups per column of the extremes kernel's grid, at most

static_assert(BH_DIAG_STRANDS == 16 && EV_SERIES * 2 * BH_DIAG_STRANDS == 256, "thread layout of the sum kernel");

namespace {

using namespace bhkit;

struct EvArgs {
    const double *beta;
    int64_t T, ld_t;
    int C, K;
    const int32_t *ladder;    // [C]
    const int32_t *start;     // [K + 1]
    const int32_t *member;    // [C], ascending within a ladder
    const void *x;            // the likes
    int64_t ldx_t, ldx_c;
    int32_t *hold;            // [T][C], contiguous
};

// flag bits of the holder kernel ...
#define EV_BAD_BETA 1
#define EV_TIE 2
// ... and of the extremes kernel
#define EV_BAD_LIKE 1
#define EV_MOVED 2

__global__ void __launch_bounds__(256) ev_holder_kernel(EvArgs a, int *flag)
{
    const int64_t n = a.T * a.C;
    int bad = 0;
    for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < n; w += (int64_t)gridDim.x * 256) {
        const int64_t t = w / a.C;
        const int c = (int)(w - t * a.C);
        const double *row = a.beta + t * a.ld_t;
        const double b = row[c];
        if (!(fabs(b) <= 1.7976931348623157e308)) bad |= EV_BAD_BETA;
        const int k = a.ladder[c];
        const int lo = a.start[k], hi = a.start[k + 1];
        int above = 0, equal = 0;
        for (int j = lo; j < hi; ++j) {
            const double bm = row[a.member[j]];
            above += bm > b ? 1 : 0;
            equal += bm == b ? 1 : 0;
        }
        if (equal > 1) bad |= EV_TIE;
        a.hold[t * a.C + lo + above] = c;     // above <= hi - lo - 1: inside the ladder's own elements, whatever the betas are
    }
    if (bad) atomicOr(flag, bad);
}

template <typename T> __device__ __forceinline__ double like_at(const EvArgs &a, int64_t t, int c)
{
    return (double)((const T *)a.x)[t * a.ldx_t + (int64_t)c * a.ldx_c];
}

// part[by][2][C]: the largest and the smallest like of the rows the workgroup (bx, by) takes
template <typename T> __global__ void __launch_bounds__(256) ev_extremes_kernel(EvArgs a, double *part, int *flag)
{
    __shared__ double red[2][4][64];
    const int jl = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + jl;
    double mx = -INFINITY, mn = INFINITY;
    int bad = 0;
    if (j < a.C) {
        const unsigned long long b0 = (unsigned long long)__double_as_longlong(a.beta[a.hold[j]]);
        for (int64_t t = (int64_t)blockIdx.y * 4 + w; t < a.T; t += 4 * (int64_t)gridDim.y) {
            const int c = a.hold[t * a.C + j];
            const double l = like_at<T>(a, t, c);
            if (!(fabs(l) <= 1.7976931348623157e308)) bad |= EV_BAD_LIKE;
            if ((unsigned long long)__double_as_longlong(a.beta[t * a.ld_t + c]) != b0) bad |= EV_MOVED;
            mx = l > mx ? l : mx;
            mn = l < mn ? l : mn;
        }
    }
    red[0][w][jl] = mx;
    red[1][w][jl] = mn;
    __syncthreads();
    if (w == 0 && j < a.C) {
        for (int i = 1; i < 4; ++i) {
            mx = red[0][i][jl] > mx ? red[0][i][jl] : mx;
            mn = red[1][i][jl] < mn ? red[1][i][jl] : mn;
        }
        part[((size_t)blockIdx.y * 2) * a.C + j] = mx;
        part[((size_t)blockIdx.y * 2 + 1) * a.C + j] = mn;
    }
    if (bad) atomicOr(flag, bad);
}

// out[3][C]: rung_beta, mx, mn for the host;  par[C][4] = mx, mn, Df, Dr for the sum kernel.  edge[j]: bit 0 = series j is a
// ladder's rung 0, bit 1 = its hottest rung
__global__ void __launch_bounds__(64) ev_extremes_finish_kernel(EvArgs a, const double *part, int nby, const unsigned char *edge, double *out,
                                                                double *par)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= a.C) return;
    double mx = -INFINITY, mn = INFINITY;
    for (int by = 0; by < nby; ++by) {
        const double u = part[((size_t)by * 2) * a.C + j], v = part[((size_t)by * 2 + 1) * a.C + j];
        mx = u > mx ? u : mx;
        mn = v < mn ? v : mn;
    }
    const double b = a.beta[a.hold[j]];
    out[j] = b;
    out[(size_t)a.C + j] = mx;
    out[2 * (size_t)a.C + j] = mn;
    par[4 * (size_t)j] = mx;
    par[4 * (size_t)j + 1] = mn;
    par[4 * (size_t)j + 2] = (edge[j] & 1) ? 0.0 : a.beta[a.hold[j - 1]] - b;
    par[4 * (size_t)j + 3] = (edge[j] & 2) ? 0.0 : b - a.beta[a.hold[j + 1]];
}

// glibc's exp for a <= 0 as the contract states it: the table path, 1 + a below 2^-54, exactly 0 at and below -BH_EVIDENCE_DROP
__device__ __forceinline__ double ev_exp(double v, const uint64_t *tab)
{
    double r = bhp_exp_core(v, tab);     // branch-free main path; meaningless outside its domain
    if (!bhp_exp_in_domain(v)) r = v <= -(double)BH_EVIDENCE_DROP ? 0.0 : 1.0 + v;
    return r;
}

__device__ __forceinline__ double ev_tree(const double (*p)[EV_SERIES], int q)
{
    return (((p[0][q] + p[1][q]) + (p[2][q] + p[3][q])) + ((p[4][q] + p[5][q]) + (p[6][q] + p[7][q]))) +
           (((p[8][q] + p[9][q]) + (p[10][q] + p[11][q])) + ((p[12][q] + p[13][q]) + (p[14][q] + p[15][q])));
}

// par[C][4] = mx, mn, Df, Dr;  out[C][4] = Sf, Sf2, Sr, Sr2.  Thread (series, direction, strand): the forward and the reverse sums of
// a series are two threads' -- they read the same hold and the same like (one address, one fetch).
template <typename T> __global__ void __launch_bounds__(256) ev_sum_kernel(EvArgs a, const double *par, double *out)
{
    __shared__ uint64_t tab[256];
    __shared__ double part[4][BH_DIAG_STRANDS][EV_SERIES];
    const int tid = threadIdx.x, jl = tid & (EV_SERIES - 1), dir = (tid >> 3) & 1, s = tid >> 4;
    const int j = blockIdx.x * EV_SERIES + jl;
    tab[tid] = bhp_exp_tab[tid];
    __syncthreads();
    double acc = 0.0, acc2 = 0.0;
    if (j < a.C) {
        const double m = par[4 * (size_t)j + dir], d = dir ? -par[4 * (size_t)j + 3] : par[4 * (size_t)j + 2];
        for (int64_t t0 = s; t0 < a.T; t0 += BH_DIAG_STRANDS * EV_FLIGHT) {
            int c[EV_FLIGHT];
            double w[EV_FLIGHT];
#pragma unroll
            for (int i = 0; i < EV_FLIGHT; ++i) {
                const int64_t t = t0 + (int64_t)i * BH_DIAG_STRANDS;
                c[i] = t < a.T ? a.hold[t * a.C + j] : 0;
            }
#pragma unroll
            for (int i = 0; i < EV_FLIGHT; ++i) {
                const int64_t t = t0 + (int64_t)i * BH_DIAG_STRANDS;
                w[i] = t < a.T ? like_at<T>(a, t, c[i]) : m;
            }
            // the rows' terms are independent of one another (a row beyond T: exp(0), not added) ...
#pragma unroll
            for (int i = 0; i < EV_FLIGHT; ++i) w[i] = ev_exp(d * (w[i] - m), tab);
            // ... and are added in ascending t
#pragma unroll
            for (int i = 0; i < EV_FLIGHT; ++i) {
                if (t0 + (int64_t)i * BH_DIAG_STRANDS < a.T) {
                    acc += w[i];
                    acc2 += w[i] * w[i];
                }
            }
        }
    }
    part[2 * dir][s][jl] = acc;
    part[2 * dir + 1][s][jl] = acc2;
    __syncthreads();
    if (tid < 4 * EV_SERIES) {
        const int q = tid >> 3, jo = tid & (EV_SERIES - 1), jj = blockIdx.x * EV_SERIES + jo;
        if (jj < a.C) out[4 * (size_t)jj + q] = ev_tree(part[q], jo);
    }
}

// the caller's hold of a BH_DEVICE call, filled from the call's own table -- unless a pass has refused the data (*refused)
__global__ void __launch_bounds__(256) ev_copy_hold_kernel(const int32_t *src, int64_t T, int C, int32_t *dst, int64_t ld, const int *refused)
{
    if (refused[0] | refused[1]) return;
    const int64_t n = T * C;
    for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < n; w += (int64_t)gridDim.x * 256) {
        const int64_t t = w / C;
        dst[t * ld + (w - t * C)] = src[w];
    }
}

struct EvCall {
    int memspace;
    int64_t T, ld_t;
    int C, K, R;
    const double *beta;
    bool sums;                // bh_chain_ladder_evidence (else the holders alone)
    int elem_bytes;
    int64_t ldx_t, ldx_c;
    const void *x;
    int32_t *hold;
    int64_t ld_hold;
    double *rung_beta, *mx, *mn, *sf, *sf2, *sr, *sr2;
};

int evidence_run(bh_engine *e, hipStream_t st, const EvCall &q, const int32_t *ladder, const std::vector<int32_t> &start,
                 const std::vector<int32_t> &member)
{
    int rc;
    const bool host = q.memspace != BH_DEVICE;
    const int C = q.C, K = q.K;
    const int64_t T = q.T;
    const size_t n = (size_t)T * (size_t)C;
    Buf cbeta, cx, work;
    EvArgs a;
    a.T = T; a.ld_t = q.ld_t; a.C = C; a.K = K; a.x = q.x; a.ldx_t = q.ldx_t; a.ldx_c = q.ldx_c;
    if ((rc = stage(e, st, q.memspace, q.beta, ((size_t)(T - 1) * (size_t)q.ld_t + (size_t)C) * 8, cbeta, &a.beta))) return rc;
    if (q.sums) {
        const size_t xspan = ((size_t)(T - 1) * (size_t)q.ldx_t + (size_t)(C - 1) * (size_t)q.ldx_c + 1) * (size_t)q.elem_bytes;
        if ((rc = stage(e, st, q.memspace, q.x, xspan, cx, &a.x))) return rc;
    }
    const int nby = (int)std::min<int64_t>((T + 3) / 4, EV_ROWBLOCKS);
    // one allocation: the ladders' tables, the flags of the two checking passes, the partials, the results, and the call's own hold
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
    const size_t o_lad = take((size_t)C * 4), o_start = take((size_t)(K + 1) * 4), o_mem = take((size_t)C * 4), o_edge = take((size_t)C),
                 o_flag = take(8), o_part = take((size_t)nby * 2 * C * 8), o_ext = take((size_t)C * 24), o_par = take((size_t)C * 32),
                 o_sum = take((size_t)C * 32), o_hold = take(n * 4);
    if ((rc = alloc(e, work, off))) return rc;
    char *w = work.as<char>();
    int *dflag = (int *)(w + o_flag);
    double *dpart = (double *)(w + o_part), *dext = (double *)(w + o_ext), *dpar = (double *)(w + o_par), *dsum = (double *)(w + o_sum);
    std::vector<unsigned char> edge(C, 0);
    for (int k = 0; k < K; ++k) {
        edge[start[k]] |= 1;
        edge[start[k + 1] - 1] |= 2;
    }
    BH_CHK(e, hipMemcpyAsync(w + o_lad, ladder, (size_t)C * 4, hipMemcpyHostToDevice, st));
    BH_CHK(e, hipMemcpyAsync(w + o_start, start.data(), (size_t)(K + 1) * 4, hipMemcpyHostToDevice, st));
    BH_CHK(e, hipMemcpyAsync(w + o_mem, member.data(), (size_t)C * 4, hipMemcpyHostToDevice, st));
    BH_CHK(e, hipMemcpyAsync(w + o_edge, edge.data(), (size_t)C, hipMemcpyHostToDevice, st));
    BH_CHK(e, hipMemsetAsync(dflag, 0, 8, st));
    // hold starts as chain 0 everywhere: where tied betas leave an element without a writer, the later passes still read inside the
    // tables -- they run without waiting for the first pass's verdict, and the flags are read once, at the end
    BH_CHK(e, hipMemsetAsync(w + o_hold, 0, n * 4, st));
    a.ladder = (const int32_t *)(w + o_lad); a.start = (const int32_t *)(w + o_start); a.member = (const int32_t *)(w + o_mem);
    a.hold = (int32_t *)(w + o_hold);
    const unsigned nblk = (unsigned)std::min<size_t>((n + 255) / 256, 16384);     // the rest by the grid's stride
    ev_holder_kernel<<<dim3(nblk), 256, 0, st>>>(a, dflag);
    BH_CHK(e, hipGetLastError());
    const dim3 grid((unsigned)((C + 63) / 64), (unsigned)nby);
    if (q.sums) {
        if (q.elem_bytes == 4) ev_extremes_kernel<float><<<grid, 256, 0, st>>>(a, dpart, dflag + 1);
        else ev_extremes_kernel<double><<<grid, 256, 0, st>>>(a, dpart, dflag + 1);
    } else {
        // the holders alone: the constancy of the betas by the same kernel, on the betas themselves as the table of likes
        EvArgs b = a;
        b.x = a.beta; b.ldx_t = a.ld_t; b.ldx_c = 1;
        ev_extremes_kernel<double><<<grid, 256, 0, st>>>(b, dpart, dflag + 1);
    }
    BH_CHK(e, hipGetLastError());
    ev_extremes_finish_kernel<<<dim3((unsigned)((C + 63) / 64)), 64, 0, st>>>(a, dpart, nby, (const unsigned char *)(w + o_edge), dext, dpar);
    BH_CHK(e, hipGetLastError());
    std::vector<double> ext((size_t)C * 3), sums((size_t)C * 4);
    if (q.sums) {
        const unsigned nb = (unsigned)((C + EV_SERIES - 1) / EV_SERIES);
        if (q.elem_bytes == 4) ev_sum_kernel<float><<<dim3(nb), 256, 0, st>>>(a, dpar, dsum);
        else ev_sum_kernel<double><<<dim3(nb), 256, 0, st>>>(a, dpar, dsum);
        BH_CHK(e, hipGetLastError());
        BH_CHK(e, hipMemcpyAsync(sums.data(), dsum, (size_t)C * 32, hipMemcpyDeviceToHost, st));
    }
    if (q.hold && !host) {      // (the kernel looks at the flags itself: a refusal leaves the caller's table as it is)
        ev_copy_hold_kernel<<<dim3(nblk), 256, 0, st>>>(a.hold, T, C, q.hold, q.ld_hold, dflag);
        BH_CHK(e, hipGetLastError());
    }
    int flag[2] = {0, 0};
    BH_CHK(e, hipMemcpyAsync(ext.data(), dext, (size_t)C * 24, hipMemcpyDeviceToHost, st));
    BH_CHK(e, hipMemcpyAsync(flag, dflag, 8, hipMemcpyDeviceToHost, st));
    BH_CHK(e, hipStreamSynchronize(st));
    if (flag[0] & EV_BAD_BETA) return fail(e, BH_EINVAL, "a beta is not finite");
    if (flag[0] & EV_TIE) return fail(e, BH_EINVAL, "tied betas: two chains of a ladder hold the same beta at some row");
    if (flag[1] & EV_BAD_LIKE) return fail(e, BH_EINVAL, "a like is not finite");
    if (flag[1] & EV_MOVED)
        return fail(e, BH_EINVAL, "the betas of a ladder change within the rows (a phase in which the ladder adaptation moved them)");
    if (q.hold && host) {
        BH_CHK(e, hipMemcpy2DAsync(q.hold, (size_t)q.ld_hold * 4, a.hold, (size_t)C * 4, (size_t)C * 4, (size_t)T, hipMemcpyDeviceToHost, st));
        BH_CHK(e, hipStreamSynchronize(st));
    }
    std::copy(ext.begin(), ext.begin() + C, q.rung_beta);
    if (q.sums) {
        std::copy(ext.begin() + C, ext.begin() + 2 * (size_t)C, q.mx);
        std::copy(ext.begin() + 2 * (size_t)C, ext.end(), q.mn);
        for (int j = 0; j < C; ++j) {
            q.sf[j] = sums[4 * (size_t)j];
            q.sf2[j] = sums[4 * (size_t)j + 1];
            q.sr[j] = sums[4 * (size_t)j + 2];
            q.sr2[j] = sums[4 * (size_t)j + 3];
        }
    }
    return BH_OK;
}

int evidence_call(bh_engine *e, void *stream, const EvCall &q, const int32_t *ladder)
{
    if (!e) return BH_EINVAL;
    if (!q.beta || !ladder || !q.rung_beta || (!q.sums && !q.hold)) return fail(e, BH_EINVAL, "null argument");
    if (q.sums && (!q.x || !q.mx || !q.mn || !q.sf || !q.sf2 || !q.sr || !q.sr2)) return fail(e, BH_EINVAL, "null argument");
    if (q.sums && q.elem_bytes != 4 && q.elem_bytes != 8) return fail(e, BH_EINVAL, "the likes must be float32 or float64");
    const int64_t T = q.T;
    const int C = q.C, K = q.K;
    if (T < 1 || C < 1 || K < 1 || K > C || q.ld_t < C || (q.hold && q.ld_hold < C) || (q.sums && (q.ldx_t < 1 || q.ldx_c < 1)))
        return fail(e, BH_EINVAL, "bad T, C, K or leading dimensions");
    bh_chain_refusal no;
    if ((no = bh_chain_ladder_span(T, q.ld_t, 0, 0)).code || (q.hold && (no = bh_chain_ladder_span(T, q.ld_hold, 0, 0)).code) ||
        (q.sums && (no = bh_chain_ladder_span(T, q.ldx_t, C, q.ldx_c)).code))
        return fail(e, no.code, no.text);
    std::vector<int32_t> start(K + 1), member(C);
    if ((no = bh_chain_ladder_groups(C, ladder, K, &q.R, start.data(), member.data(), nullptr)).code) return fail(e, no.code, no.text);
    hipError_t he = hipSetDevice(bh_engine_device_internal(e));
    if (he != hipSuccess) return fail(e, BH_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(he));
    hipStream_t st = call_stream(e, q.memspace, stream);
    const int rc = evidence_run(e, st, q, ladder, start, member);
    if (rc != BH_OK) (void)hipStreamSynchronize(st);   // (the buffers go with that frame)
    return rc;
}

} // namespace

extern "C" {

int bh_chain_ladder_holders(bh_engine *e, int memspace, void *stream, int64_t T, int C, int64_t ld_t, const double *beta,
                            const int32_t *ladder, int K, int R, int32_t *hold, int64_t ld_hold, double *rung_beta)
{
    EvCall q{};
    q.memspace = memspace; q.T = T; q.ld_t = ld_t; q.C = C; q.K = K; q.R = R; q.beta = beta; q.sums = false;
    q.hold = hold; q.ld_hold = ld_hold; q.rung_beta = rung_beta;
    return evidence_call(e, stream, q, ladder);
}

int bh_chain_ladder_evidence(bh_engine *e, int memspace, void *stream, int64_t T, int C, int64_t ld_t, const double *beta,
                             int elem_bytes, int64_t ldx_t, int64_t ldx_c, const void *x, const int32_t *ladder, int K, int R,
                             int32_t *hold, int64_t ld_hold, double *rung_beta, double *mx, double *mn, double *sf, double *sf2,
                             double *sr, double *sr2)
{
    EvCall q{};
    q.memspace = memspace; q.T = T; q.ld_t = ld_t; q.C = C; q.K = K; q.R = R; q.beta = beta; q.sums = true;
    q.elem_bytes = elem_bytes; q.ldx_t = ldx_t; q.ldx_c = ldx_c; q.x = x;
    q.hold = hold; q.ld_hold = ld_hold; q.rung_beta = rung_beta; q.mx = mx; q.mn = mn; q.sf = sf; q.sf2 = sf2; q.sr = sr; q.sr2 = sr2;
    return evidence_call(e, stream, q, ladder);
}

} // extern "C"
