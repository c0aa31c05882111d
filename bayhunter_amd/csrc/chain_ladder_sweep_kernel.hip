// bayhunter_amd/csrc/chain_ladder_sweep_kernel.hip -- the swap sweep of tempered chains (include/bh_engine_chain_ladder_sweep.h).
//
// One wavefront per ladder (a ladder has at most 64 chains), a workgroup of one wavefront: every branch below that holds a barrier is
// taken by the whole workgroup.  Lane j is first the j-th member of its ladder in ascending chain order: it counts its rung over the
// members' betas in one LDS row (larger betas, and equal ones of earlier members) and leaves (beta, like, chain) at that rung.  From there lane p is POSITION p: the pair (p, p+1), rung p
// of the sorted ladder, chain order[p].  Every counter and every beta has exactly one writing lane; there are no atomics.
// The two sums and the recurrence of the adaptation are serial, in ascending order (the order is the contract): every lane runs
// them on the same LDS rows (same address in all lanes: a broadcast), so every lane holds the same bits and no result is passed on.
// The betas are read before the first barrier and written after the last; ladders share no chain.
#include "bh_hostkit.h"
#include "chain_tables.h"
#include "../../include/bh_engine_chain_ladder_sweep.h"

#include <algorithm>
#include <cstdint>
#include <new>
#include <string>
#include <vector>

struct bh_ladder_sweep {
    int C = 0, K = 0;
    int32_t *start = nullptr, *member = nullptr;          // [K + 1], [C]
    long long *proposed = nullptr, *accepted = nullptr;   // [2][C]
    long long *wprop = nullptr, *wacc = nullptr;          // [C]
    long long *adaptations = nullptr, *skipped = nullptr; // [K]
    double *rung_beta = nullptr;                          // [C]
    hipStream_t last = nullptr;                           // the stream of the last sweep
    bool ran = false;
};

namespace {

struct SweepArgs {
    int C, K;
    const int32_t *start, *member;
    long long *proposed, *accepted, *wprop, *wacc, *adaptations, *skipped;
    double *rung_beta;
    const double *like, *logu;
    double *beta;
    int parity, phase, adapt;
    double kappa;
};

__global__ void __launch_bounds__(64) ladder_sweep_kernel(SweepArgs a)
{
    __shared__ double B[64], L[64], X[64];
    __shared__ int Cn[64];
    const int lane = threadIdx.x, k = blockIdx.x;    // k < K: the grid
    const int lo = a.start[k];
    const int R = a.start[k + 1] - lo;               // 1..64

    // ---- 1. order: a lane per member
    int c = 0;
    double bj = 0.0, lj = 0.0;
    Cn[lane] = -1;      // (betas that are NaN share rung 0 and leave rungs without a chain: such a rung writes no beta)
    if (lane < R) {
        c = a.member[lo + lane];                     // < C (bh_ladder_sweep_create)
        bj = a.beta[c];
        lj = a.like[c];
        X[lane] = bj;
    }
    __syncthreads();
    if (lane < R) {
        int rung = 0;
        for (int i = 0; i < R; ++i) {
            const double bi = X[i];
            rung += (bi > bj || (bi == bj && i < lane)) ? 1 : 0;
        }
        B[rung] = bj; L[rung] = lj; Cn[rung] = c;     // rung < R: the member itself is never counted
    }
    __syncthreads();

    // ---- 2. decide: a lane per position
    const int p = lane;
    const bool pair = p + 1 < R && (p & 1) == a.parity;
    bool acc = false;
    double b0 = 0.0;
    if (p < R) b0 = B[p];
    if (pair) {
        const double b1 = B[p + 1], l0 = L[p], l1 = L[p + 1];
        acc = a.logu[lo + p] < (b0 - b1) * (l1 - l0);
    }
    const unsigned long long accmask = __ballot(acc);
    int q = p;                                       // the rung that chain order[p] holds after the swaps
    if (acc) q = p + 1;
    else if (p >= 1 && ((accmask >> (p - 1)) & 1ull)) q = p - 1;

    long long wp = 0, wa = 0;
    if (p + 1 < R) {
        wp = a.wprop[lo + p] + (pair ? 1 : 0);
        wa = a.wacc[lo + p] + (acc ? 1 : 0);
        if (pair) {
            a.proposed[(size_t)a.phase * a.C + lo + p] += 1;
            if (acc) a.accepted[(size_t)a.phase * a.C + lo + p] += 1;
        }
    }

    // ---- 3. adapt
    const bool adapting = a.adapt != 0 && R >= 3;    // (the same in every lane)
    bool moved = false;
    double mine = 0.0, sorted = b0;                   // mine: nb[q]; sorted: nb[p]
    if (adapting) {
        const bool empty = __ballot(p + 1 < R && wp == 0) != 0ull;
        if (!empty) {                                 // (the same in every lane)
            if (p + 1 < R) X[p] = (double)wa / (double)wp;
            __syncthreads();
            double sum = 0.0;
            for (int i = 0; i + 1 < R; ++i) sum += X[i];
            const double abar = sum / (double)(R - 1);
            const double span = B[0] - B[R - 1];
            const double floor_ = 0x1p-20 * span;
            double g1 = 0.0;
            if (p + 1 < R) {
                const double x = (b0 - B[p + 1]) * (1.0 + a.kappa * (X[p] - abar));
                g1 = x > floor_ ? x : floor_;
            }
            __syncthreads();
            if (p + 1 < R) X[p] = g1;
            __syncthreads();
            double s = 0.0;
            for (int i = 0; i + 1 < R; ++i) s += X[i];
            const double g2 = (g1 * span) / s;
            __syncthreads();
            if (p + 1 < R) X[p] = g2;
            __syncthreads();
            double nb = B[0];
            bool strict = true;
            if (q == 0) mine = nb;
            if (p == 0) sorted = nb;
            for (int r = 1; r < R; ++r) {
                const double next = r == R - 1 ? B[R - 1] : nb - X[r - 1];
                strict = strict && nb > next;
                nb = next;
                if (q == r) mine = nb;
                if (p == r) sorted = nb;
            }
            moved = strict;
        }
        wp = 0; wa = 0;
        if (p == 0) {
            if (moved) a.adaptations[k] += 1;
            else a.skipped[k] += 1;
        }
    }
    if (p + 1 < R) {
        a.wprop[lo + p] = wp;
        a.wacc[lo + p] = wa;
    }
    if (p < R) {
        if (!moved) { mine = B[q]; sorted = b0; }
        const int cp = Cn[p];
        if (cp >= 0) a.beta[cp] = mine;
        a.rung_beta[lo + p] = sorted;
    }
}

using bhkit::fail;

void release(bh_ladder_sweep *p)
{
    void *bufs[] = {p->start, p->member, p->proposed, p->accepted, p->wprop, p->wacc, p->adaptations, p->skipped, p->rung_beta};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    delete p;
}

template <typename T> int zalloc(bh_engine *e, T *&p, size_t n)
{
    hipError_t he = hipMalloc((void **)&p, n * sizeof(T));
    if (he != hipSuccess) { p = nullptr; return fail(e, BH_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(he)); }
    he = hipMemset(p, 0, n * sizeof(T));
    if (he != hipSuccess) return fail(e, BH_EHIP, std::string("hipMemset: ") + hipGetErrorString(he));
    return BH_OK;
}

} // namespace

extern "C" {

int bh_ladder_sweep_create(bh_engine *e, int C, const int32_t *ladder, int K, bh_ladder_sweep **plan)
{
    if (!e) return BH_EINVAL;
    if (!ladder || !plan) return fail(e, BH_EINVAL, "null argument");
    if (C < 1 || K < 1 || K > C) return fail(e, BH_EINVAL, "bad C or K");
    std::vector<int32_t> start(K + 1), member(C);
    const bh_chain_refusal no = bh_chain_ladder_groups(C, ladder, K, nullptr, start.data(), member.data(), nullptr);
    if (no.code) return fail(e, no.code, no.text);
    BH_CHK(e, hipSetDevice(bh_engine_device_internal(e)));
    bh_ladder_sweep *p = new (std::nothrow) bh_ladder_sweep;
    if (!p) return fail(e, BH_ENOMEM, "out of host memory");
    p->C = C; p->K = K;
    int rc;
    if ((rc = zalloc(e, p->start, (size_t)K + 1)) || (rc = zalloc(e, p->member, (size_t)C)) ||
        (rc = zalloc(e, p->proposed, (size_t)2 * C)) || (rc = zalloc(e, p->accepted, (size_t)2 * C)) ||
        (rc = zalloc(e, p->wprop, (size_t)C)) || (rc = zalloc(e, p->wacc, (size_t)C)) || (rc = zalloc(e, p->adaptations, (size_t)K)) ||
        (rc = zalloc(e, p->skipped, (size_t)K)) || (rc = zalloc(e, p->rung_beta, (size_t)C))) {
        release(p);
        return rc;
    }
    hipError_t he = hipMemcpy(p->start, start.data(), ((size_t)K + 1) * 4, hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(p->member, member.data(), (size_t)C * 4, hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipDeviceSynchronize();     // (the zeros and the lists are there before any stream reads them)
    if (he != hipSuccess) {
        release(p);
        return fail(e, BH_EHIP, std::string("hipMemcpy: ") + hipGetErrorString(he));
    }
    *plan = p;
    return BH_OK;
}

int bh_ladder_sweep_run(bh_engine *e, bh_ladder_sweep *plan, void *stream, const double *like, double *beta, const double *logu,
                        int parity, int phase, int adapt, double kappa)
{
    if (!e) return BH_EINVAL;
    if (!plan || !like || !beta || !logu) return fail(e, BH_EINVAL, "null argument");
    if ((parity != 0 && parity != 1) || (phase != 0 && phase != 1)) return fail(e, BH_EINVAL, "parity and phase are 0 or 1");
    if (adapt != 0 && phase == 1) return fail(e, BH_EINVAL, "the temperatures of the main phase are frozen: adapt with phase 1");
    BH_CHK(e, hipSetDevice(bh_engine_device_internal(e)));
    hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)bh_engine_stream(e);
    SweepArgs a;
    a.C = plan->C; a.K = plan->K; a.start = plan->start; a.member = plan->member;
    a.proposed = plan->proposed; a.accepted = plan->accepted; a.wprop = plan->wprop; a.wacc = plan->wacc;
    a.adaptations = plan->adaptations; a.skipped = plan->skipped; a.rung_beta = plan->rung_beta;
    a.like = like; a.logu = logu; a.beta = beta;
    a.parity = parity; a.phase = phase; a.adapt = adapt; a.kappa = kappa;
    ladder_sweep_kernel<<<dim3((unsigned)plan->K), 64, 0, st>>>(a);
    BH_CHK(e, hipGetLastError());
    plan->last = st;
    plan->ran = true;
    return BH_OK;
}

int bh_ladder_sweep_read(bh_engine *e, bh_ladder_sweep *plan, int64_t *proposed, int64_t *accepted, double *rung_beta,
                         int64_t *adaptations, int64_t *skipped)
{
    if (!e) return BH_EINVAL;
    if (!plan) return fail(e, BH_EINVAL, "null argument");
    BH_CHK(e, hipSetDevice(bh_engine_device_internal(e)));
    if (plan->ran) BH_CHK(e, hipStreamSynchronize(plan->last));
    const size_t C = (size_t)plan->C, K = (size_t)plan->K;
    // into buffers of the call first: an error writes nothing to the outputs
    std::vector<int64_t> hp(2 * C), ha(2 * C), hn(K), hs(K);
    std::vector<double> hb(C);
    BH_CHK(e, hipMemcpy(hp.data(), plan->proposed, 2 * C * 8, hipMemcpyDeviceToHost));
    BH_CHK(e, hipMemcpy(ha.data(), plan->accepted, 2 * C * 8, hipMemcpyDeviceToHost));
    BH_CHK(e, hipMemcpy(hb.data(), plan->rung_beta, C * 8, hipMemcpyDeviceToHost));
    BH_CHK(e, hipMemcpy(hn.data(), plan->adaptations, K * 8, hipMemcpyDeviceToHost));
    BH_CHK(e, hipMemcpy(hs.data(), plan->skipped, K * 8, hipMemcpyDeviceToHost));
    if (proposed) std::copy(hp.begin(), hp.end(), proposed);
    if (accepted) std::copy(ha.begin(), ha.end(), accepted);
    if (rung_beta) std::copy(hb.begin(), hb.end(), rung_beta);
    if (adaptations) std::copy(hn.begin(), hn.end(), adaptations);
    if (skipped) std::copy(hs.begin(), hs.end(), skipped);
    return BH_OK;
}

int bh_ladder_sweep_destroy(bh_engine *e, bh_ladder_sweep *plan)
{
    if (!e) return BH_EINVAL;
    if (!plan) return BH_OK;
    if (plan->ran) (void)hipStreamSynchronize(plan->last);
    release(plan);
    return BH_OK;
}

} // extern "C"
