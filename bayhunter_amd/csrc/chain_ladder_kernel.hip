// bayhunter_amd/csrc/chain_ladder_kernel.hip -- the cold series of tempered runs: bh_chain_ladder_index (include/bh_engine_chain_diag_ladders.h).
//
// From the recorded betas [T][C] and the chains' ladders: the rung of every chain at every row, the chain that holds every ladder's
// largest beta (the selection the gathered diagnostics read), and the numbers that say whether the ladders mix.  All in integers.
//
// check kernel : one thread per (t, c): a beta that is not finite raises the flag; the host reads it before anything is written.
// rung kernel  : one thread per (t, c).  It compares its beta with those of its ladder's members (at most 64, listed in ascending
//                chain order; consecutive threads are consecutive chains of one row, the members' betas come from that row):
//                rung = the number of larger ones, hot = none smaller and rung > 0.  The thread with rung 0 and no equal beta
//                before it is the ladder's selection and writes sel[t][k]: one writer per (t, k), no atomics.  Every thread leaves
//                one byte code[t][c] = rung | hot << 7 for the walk, and the rung where the caller asked for it.
// walk kernel  : one lane per chain walks the codes in ascending t, 16 rows in flight; neighbouring lanes read neighbouring bytes.
//                The three-state trip count is in a register, the occupancy counts in LDS ([R][64 lanes]: a lane's own column, no
//                conflicts).
// moves kernel : one lane per ladder walks sel in ascending t and counts the changes.
#include "bh_hostkit.h"
#include "chain_tables.h"
#include "../../include/bh_engine_chain_diag_ladders.h"

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace {

using namespace bhkit;

struct LadderArgs {
    const double *beta;
    int64_t T, ld_t;
    int C, K;
    const int32_t *ladder;    // [C]
    const int32_t *start;     // [K + 1]: the members of ladder k are member[start[k] .. start[k+1])
    const int32_t *member;    // [C], ascending within a ladder
};

__global__ void __launch_bounds__(256) ladder_check_kernel(LadderArgs a, int *flag)
{
    const int64_t n = a.T * a.C;
    int bad = 0;
    for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < n; w += (int64_t)gridDim.x * 256) {
        const int64_t t = w / a.C;
        const int c = (int)(w - t * a.C);
        const double b = a.beta[t * a.ld_t + c];
        if (!(fabs(b) <= 1.7976931348623157e308)) bad = 1;
    }
    if (bad) atomicOr(flag, 1);
}

__global__ void __launch_bounds__(256) ladder_rung_kernel(LadderArgs a, int32_t *sel, int64_t ld_sel, int32_t *rung, int64_t ld_rung,
                                                          unsigned char *code)
{
    const int64_t n = a.T * a.C;
    for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < n; w += (int64_t)gridDim.x * 256) {
        const int64_t t = w / a.C;
        const int c = (int)(w - t * a.C);
        const double *row = a.beta + t * a.ld_t;
        const double b = row[c];
        const int k = a.ladder[c];
        const int lo = a.start[k], hi = a.start[k + 1];
        int above = 0, below = 0, before = 0;
        for (int j = lo; j < hi; ++j) {
            const int m = a.member[j];
            const double bm = row[m];
            above += bm > b ? 1 : 0;
            below += bm < b ? 1 : 0;
            before += (bm == b && m < c) ? 1 : 0;
        }
        const int hot = (below == 0 && above > 0) ? 1 : 0;
        code[w] = (unsigned char)(above | (hot << 7));
        if (rung) rung[t * ld_rung + c] = above;
        if (above == 0 && before == 0) sel[t * ld_sel + k] = c;
    }
}

#define LADDER_FLIGHT 16

// occupancy[c][r], round_trips[c]
__global__ void __launch_bounds__(64) ladder_walk_kernel(const unsigned char *code, int64_t T, int C, int R, unsigned long long *occupancy,
                                                         unsigned long long *trips)
{
    __shared__ unsigned long long occ[BH_LADDER_MAXRUNGS][64];
    const int lane = threadIdx.x, c = blockIdx.x * 64 + lane;
    for (int r = 0; r < R; ++r) occ[r][lane] = 0;
    if (c >= C) return;     // (a lane's column of occ is its own: no barrier)
    unsigned long long ntrips = 0;
    int state = 0;          // 0: none, 1: cold seen, 2: hot seen after cold
    for (int64_t t0 = 0; t0 < T; t0 += LADDER_FLIGHT) {
        unsigned char v[LADDER_FLIGHT];
#pragma unroll
        for (int i = 0; i < LADDER_FLIGHT; ++i) v[i] = t0 + i < T ? code[(t0 + i) * C + c] : (unsigned char)0x7f;
#pragma unroll
        for (int i = 0; i < LADDER_FLIGHT; ++i) {
            if (t0 + i < T) {
                const int r = v[i] & 0x7f, hot = v[i] >> 7;
                occ[r][lane] += 1;      // r < the ladder's size <= R
                if (r == 0) {
                    ntrips += state == 2 ? 1 : 0;
                    state = 1;
                } else if (hot && state == 1) {
                    state = 2;
                }
            }
        }
    }
    for (int r = 0; r < R; ++r) occupancy[(size_t)c * R + r] = occ[r][lane];
    trips[c] = ntrips;
}

__global__ void __launch_bounds__(64) ladder_moves_kernel(const int32_t *sel, int64_t ld_sel, int64_t T, int K, unsigned long long *moves)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= K) return;
    unsigned long long n = 0;
    int prev = sel[k];
    for (int64_t t0 = 1; t0 < T; t0 += LADDER_FLIGHT) {
        int v[LADDER_FLIGHT];
#pragma unroll
        for (int i = 0; i < LADDER_FLIGHT; ++i) v[i] = t0 + i < T ? sel[(t0 + i) * ld_sel + k] : 0;
#pragma unroll
        for (int i = 0; i < LADDER_FLIGHT; ++i) {
            if (t0 + i < T) {
                n += v[i] != prev ? 1 : 0;
                prev = v[i];
            }
        }
    }
    moves[k] = n;
}

int ladder_run(bh_engine *e, int memspace, hipStream_t st, int64_t T, int C, int64_t ld_t, const double *beta, const int32_t *ladder,
               const std::vector<int32_t> &start, const std::vector<int32_t> &member, int K, int R, int32_t *sel, int64_t ld_sel,
               int32_t *rung, int64_t ld_rung, int64_t *occupancy, int64_t *round_trips, int64_t *moves)
{
    int rc;
    const bool host = memspace != BH_DEVICE;
    const size_t n = (size_t)T * (size_t)C;
    Buf cbeta, dlad, dstart, dmem, dflag, dcode, dsel, drung, docc, dtrips, dmoves;
    LadderArgs a;
    a.T = T; a.ld_t = ld_t; a.C = C; a.K = K;
    if ((rc = stage(e, st, memspace, beta, ((size_t)(T - 1) * (size_t)ld_t + (size_t)C) * 8, cbeta, &a.beta))) return rc;
    if ((rc = alloc(e, dlad, (size_t)C * 4)) || (rc = alloc(e, dstart, (size_t)(K + 1) * 4)) || (rc = alloc(e, dmem, (size_t)C * 4)) ||
        (rc = alloc(e, dflag, 8)) || (rc = alloc(e, dcode, n)) || (rc = alloc(e, docc, (size_t)C * R * 8)) ||
        (rc = alloc(e, dtrips, (size_t)C * 8)) || (rc = alloc(e, dmoves, (size_t)K * 8)))
        return rc;
    BH_CHK(e, hipMemcpyAsync(dlad.p, ladder, (size_t)C * 4, hipMemcpyHostToDevice, st));
    BH_CHK(e, hipMemcpyAsync(dstart.p, start.data(), (size_t)(K + 1) * 4, hipMemcpyHostToDevice, st));
    BH_CHK(e, hipMemcpyAsync(dmem.p, member.data(), (size_t)C * 4, hipMemcpyHostToDevice, st));
    BH_CHK(e, hipMemsetAsync(dflag.p, 0, 8, st));
    a.ladder = dlad.as<int32_t>(); a.start = dstart.as<int32_t>(); a.member = dmem.as<int32_t>();
    const unsigned nblk = (unsigned)std::min<size_t>((n + 255) / 256, 16384);     // the rest by the grid's stride
    ladder_check_kernel<<<dim3(nblk), 256, 0, st>>>(a, dflag.as<int>());
    BH_CHK(e, hipGetLastError());
    int flag = 0;
    BH_CHK(e, hipMemcpyAsync(&flag, dflag.p, 4, hipMemcpyDeviceToHost, st));
    BH_CHK(e, hipStreamSynchronize(st));
    if (flag) return fail(e, BH_EINVAL, "a beta is not finite");
    // a host call's sel and rung: contiguous on the device, copied back row by row
    int32_t *ksel = sel, *krung = rung;
    int64_t kld_sel = ld_sel, kld_rung = ld_rung;
    if (host) {
        if ((rc = alloc(e, dsel, (size_t)T * K * 4))) return rc;
        ksel = dsel.as<int32_t>(); kld_sel = K;
        if (rung) {
            if ((rc = alloc(e, drung, n * 4))) return rc;
            krung = drung.as<int32_t>(); kld_rung = C;
        }
    }
    ladder_rung_kernel<<<dim3(nblk), 256, 0, st>>>(a, ksel, kld_sel, krung, kld_rung, dcode.as<unsigned char>());
    BH_CHK(e, hipGetLastError());
    ladder_walk_kernel<<<dim3((unsigned)((C + 63) / 64)), 64, 0, st>>>(dcode.as<unsigned char>(), T, C, R, docc.as<unsigned long long>(),
                                                                      dtrips.as<unsigned long long>());
    BH_CHK(e, hipGetLastError());
    ladder_moves_kernel<<<dim3((unsigned)((K + 63) / 64)), 64, 0, st>>>(ksel, kld_sel, T, K, dmoves.as<unsigned long long>());
    BH_CHK(e, hipGetLastError());
    std::vector<int64_t> hocc((size_t)C * R), htrips(C), hmoves(K);
    BH_CHK(e, hipMemcpyAsync(hocc.data(), docc.p, hocc.size() * 8, hipMemcpyDeviceToHost, st));
    BH_CHK(e, hipMemcpyAsync(htrips.data(), dtrips.p, (size_t)C * 8, hipMemcpyDeviceToHost, st));
    BH_CHK(e, hipMemcpyAsync(hmoves.data(), dmoves.p, (size_t)K * 8, hipMemcpyDeviceToHost, st));
    if (host) {
        BH_CHK(e, hipMemcpy2DAsync(sel, (size_t)ld_sel * 4, ksel, (size_t)K * 4, (size_t)K * 4, (size_t)T, hipMemcpyDeviceToHost, st));
        if (rung)
            BH_CHK(e, hipMemcpy2DAsync(rung, (size_t)ld_rung * 4, krung, (size_t)C * 4, (size_t)C * 4, (size_t)T, hipMemcpyDeviceToHost, st));
    }
    BH_CHK(e, hipStreamSynchronize(st));
    std::copy(hocc.begin(), hocc.end(), occupancy);
    std::copy(htrips.begin(), htrips.end(), round_trips);
    std::copy(hmoves.begin(), hmoves.end(), moves);
    return BH_OK;
}

} // namespace

extern "C" {

int bh_chain_ladder_index(bh_engine *e, int memspace, void *stream, int64_t T, int C, int64_t ld_t, const double *beta,
                          const int32_t *ladder, int K, int R, int32_t *sel, int64_t ld_sel, int32_t *rung, int64_t ld_rung,
                          int64_t *occupancy, int64_t *round_trips, int64_t *moves)
{
    if (!e) return BH_EINVAL;
    if (!beta || !ladder || !sel || !occupancy || !round_trips || !moves) return fail(e, BH_EINVAL, "null argument");
    if (T < 1 || C < 1 || K < 1 || K > C || ld_t < C || ld_sel < K || (rung && ld_rung < C))
        return fail(e, BH_EINVAL, "bad T, C, K or leading dimensions");
    bh_chain_refusal no;
    if ((no = bh_chain_ladder_span(T, ld_t, 0, 0)).code || (no = bh_chain_ladder_span(T, ld_sel, 0, 0)).code ||
        (rung && (no = bh_chain_ladder_span(T, ld_rung, 0, 0)).code))
        return fail(e, no.code, no.text);
    std::vector<int32_t> start(K + 1), member(C);
    if ((no = bh_chain_ladder_groups(C, ladder, K, &R, start.data(), member.data(), nullptr)).code) return fail(e, no.code, no.text);
    hipError_t he = hipSetDevice(bh_engine_device_internal(e));
    if (he != hipSuccess) return fail(e, BH_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(he));
    hipStream_t st = call_stream(e, memspace, stream);
    const int rc = ladder_run(e, memspace, st, T, C, ld_t, beta, ladder, start, member, K, R, sel, ld_sel, rung, ld_rung, occupancy,
                              round_trips, moves);
    if (rc != BH_OK) (void)hipStreamSynchronize(st);   // (the buffers go with that frame)
    return rc;
}

} // extern "C"
