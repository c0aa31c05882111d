// bayhunter_amd/csrc/posterior_classes_kernel.hip -- every loaded row's class by a rule over the columns of the scalar sets, and
// a set's columns by input row (include/bh_engine_posterior_classes.h).
//
// One lane per loaded row, as the kernels that form the sets.  The term table is the same for every lane: the loop over it is
// uniform (scalar loads of the term, one coalesced load of the term's column per wavefront) and a lane only stops looking once
// its class is known; a (site, term)'s bounds are read at the row's own site -- rows lie grouped by site, so all but the
// wavefronts that straddle a site boundary read one address.  The class goes to the row's index in the loaded input with a
// plain vector store; cls was filled with -1 by a launch before, which is what a row the load left out keeps.  Counts: the rows
// of a workgroup belong to the site of its first row, to that of its last, or (sites of fewer rows than a workgroup) to one
// between; the first two count in LDS and flush one 64-bit integer atomic per non-empty (site, class), the rest meet in the
// wave-aggregated atomics of posterior_common.h.  Integer sums: exact in any order.
#include "posterior_common.h"
#include "../../include/bh_engine_posterior_classes.h"

#include <cmath>

using namespace bhpost;

namespace {

#define PC_SLOTS (BH_CLASSES_MAX + 1)

struct PcTerm {
    const double *col;   // the term's column over the loaded rows
    int32_t cls, op;
};

__global__ void __launch_bounds__(256) pc_fill_kernel(int64_t N, int32_t *cls)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) cls[i] = -1;
}

__global__ void __launch_bounds__(256) pc_classes_kernel(int64_t nrows, const int32_t *__restrict__ psite,
                                                         const int64_t *__restrict__ porig, int K, int T,
                                                         const PcTerm *__restrict__ term, const double *__restrict__ lo,
                                                         const double *__restrict__ hi, int32_t *__restrict__ cls,
                                                         unsigned long long *counts)
{
    __shared__ unsigned int lc[2 * PC_SLOTS];
    const int64_t b0 = (int64_t)blockIdx.x * blockDim.x, r = b0 + threadIdx.x;
    const int64_t bl = b0 + blockDim.x - 1 < nrows - 1 ? b0 + blockDim.x - 1 : nrows - 1;
    const int sa = psite[b0], sb = psite[bl];   // (b0 < nrows: the grid covers the rows and no more)
    if (threadIdx.x < 2 * PC_SLOTS) lc[threadIdx.x] = 0u;
    __syncthreads();
    const bool act = r < nrows;
    const int s = act ? psite[r] : sa;
    // res == K: not known yet, at the end: no class.  cur: the class whose terms are being read; ok: all of them held so far.
    int res = act ? K : 0, cur = 0;
    bool ok = true;
    for (int t = 0; t < T; ++t) {
        if (!__ballot(res == K)) break;
        const PcTerm tm = term[t];
        if (tm.cls != cur) {   // class cur is complete; the classes between it and the term's have no term and hold for every row
            if (res == K) res = ok ? cur : (tm.cls > cur + 1 ? cur + 1 : K);
            cur = tm.cls;
            ok = true;
        }
        if (res == K && ok) {
            const double v = tm.col[r];
            if (tm.op == BH_CLASS_IN) ok = v == v && lo[(size_t)s * T + t] <= v && v < hi[(size_t)s * T + t];
            else ok = (tm.op == BH_CLASS_HAS) == (v == v);
        }
    }
    if (res == K) res = ok ? cur : (cur + 1 < K ? cur + 1 : K);
    if (act) {
        cls[porig[r]] = res < K ? res : -1;
        if (s == sa) atomicAdd(&lc[res], 1u);
        else if (s == sb) atomicAdd(&lc[PC_SLOTS + res], 1u);
    }
    const bool between = act && s != sa && s != sb;
    if (__ballot(between)) agg_add(counts, s * (K + 1) + res, between);   // (the ballot is the wavefront's: every lane calls)
    __syncthreads();
    if (threadIdx.x < 2 * PC_SLOTS) {
        const int half = threadIdx.x / PC_SLOTS, k = threadIdx.x % PC_SLOTS;
        const unsigned int c = lc[threadIdx.x];
        if (c) atomicAdd(&counts[(size_t)(half ? sb : sa) * (K + 1) + k], (unsigned long long)c);
    }
}

// out[i * ld + q] = NaN for every input row i and column q of the set ...
__global__ void __launch_bounds__(256) pc_export_fill_kernel(int64_t N, int Q, int64_t ld, double *out)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N * Q) return;
    out[(e / Q) * ld + e % Q] = __longlong_as_double(0x7ff8000000000000ll);
}

// ... and the loaded rows' values over it: a lane per loaded row, coalesced reads of every column
__global__ void __launch_bounds__(256) pc_export_kernel(int64_t nrows, const int64_t *__restrict__ porig, int Q,
                                                        const double *__restrict__ val, int64_t ld, double *__restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    double *o = out + porig[r] * ld;
    for (int q = 0; q < Q; ++q) o[q] = val[(int64_t)q * nrows + r];
}

int formed_set(bh_posterior *p, int set, const std::string &at, ScalarSet **out)
{
    const int slot = set_slot(set);
    if (slot < 0) return pfail(p, BH_EINVAL, at + "no such scalar set");
    if (p->sets[slot].Q < 1) return pfail(p, BH_EINVAL, at + "the set does not exist yet (form it on the handle first)");
    *out = &p->sets[slot];
    return BH_OK;
}

} // namespace

extern "C" {

int bh_posterior_classes(bh_posterior *p, int K, int T, const int32_t *term_class, const int32_t *term_set,
                         const int32_t *term_col, const int32_t *term_op, const double *lo, const double *hi,
                         int memspace, void *stream, int32_t *cls, int64_t *counts)
{
    int rc;
    if (!p) return BH_EINVAL;
    if (p->S < 1) return pfail(p, BH_EINVAL, "no rows loaded (bh_posterior_load)");
    if (!p->has_rows) return pfail(p, BH_EINVAL, "the rows were loaded without bh_posterior_keep_rows");
    if (K < 1 || K > BH_CLASSES_MAX) return pfail(p, BH_EINVAL, "K: 1..BH_CLASSES_MAX (16) classes in one call");
    if (T < 0 || T > BH_CLASS_MAXTERMS) return pfail(p, BH_EINVAL, "T: 0..BH_CLASS_MAXTERMS (64) terms in one call");
    if ((T && (!term_class || !term_set || !term_col || !term_op || !lo || !hi)) || (!cls && p->ninput) || !counts)
        return pfail(p, BH_EINVAL, "null argument");
    const int S = p->S;
    std::vector<PcTerm> tab(T > 0 ? T : 1);
    for (int t = 0; t < T; ++t) {
        const std::string at = "term " + std::to_string(t) + ": ";
        if (term_class[t] < 0 || term_class[t] >= K) return pfail(p, BH_EINVAL, at + "term_class outside [0, K)");
        if (t && term_class[t] < term_class[t - 1]) return pfail(p, BH_EINVAL, at + "term_class must ascend");
        if (term_op[t] < BH_CLASS_IN || term_op[t] > BH_CLASS_LACKS) return pfail(p, BH_EINVAL, at + "no such op");
        if (term_set[t] != BH_SCALARS_MOHO && term_set[t] != BH_SCALARS_USER && term_set[t] != BH_SCALARS_FEATURES)
            return pfail(p, BH_EINVAL, at + "the set must be BH_SCALARS_MOHO, BH_SCALARS_USER or BH_SCALARS_FEATURES");
        ScalarSet *ss;
        if ((rc = formed_set(p, term_set[t], at, &ss))) return rc;
        if (term_col[t] < 0 || term_col[t] >= ss->Q) return pfail(p, BH_EINVAL, at + "column outside the set");
        if (term_op[t] == BH_CLASS_IN)
            for (int s = 0; s < S; ++s) {
                const double a = lo[(size_t)s * T + t], b = hi[(size_t)s * T + t];
                if (a != a || b != b) return pfail(p, BH_EINVAL, at + "site " + std::to_string(s) + ": a bound is NaN");
                if (a > b) return pfail(p, BH_EINVAL, at + "site " + std::to_string(s) + ": lo > hi");
            }
        tab[t] = PcTerm{ss->val.as<double>() + (int64_t)term_col[t] * p->nrows, term_class[t], term_op[t]};
    }
    PCHK(p, hipSetDevice(p->device));
    const bool host = memspace != BH_DEVICE;
    p->st = (!host && stream) ? (hipStream_t)stream : (hipStream_t)bh_engine_stream(p->e);
    const size_t nr = (size_t)p->nrows, N = (size_t)p->ninput, ncnt = (size_t)S * (K + 1), nb = (size_t)S * T;
    Dev dtab, dlo, dhi, dcnt, dcls;
    if ((rc = alloc(p, dtab, tab.size() * sizeof(PcTerm))) || (rc = alloc(p, dlo, nb * 8)) || (rc = alloc(p, dhi, nb * 8)) ||
        (rc = alloc(p, dcnt, ncnt * 8)) || (host && (rc = alloc(p, dcls, N * 4))))
        return rc;
    int32_t *c = host ? dcls.as<int32_t>() : cls;
    if (T) {
        PCHK(p, hipMemcpyAsync(dtab.p, tab.data(), (size_t)T * sizeof(PcTerm), hipMemcpyHostToDevice, p->st));
        PCHK(p, hipMemcpyAsync(dlo.p, lo, nb * 8, hipMemcpyHostToDevice, p->st));
        PCHK(p, hipMemcpyAsync(dhi.p, hi, nb * 8, hipMemcpyHostToDevice, p->st));
    }
    PCHK(p, hipMemsetAsync(dcnt.p, 0, ncnt * 8, p->st));
    if (N) {
        pc_fill_kernel<<<(unsigned)((N + 255) / 256), 256, 0, p->st>>>(p->ninput, c);
        PCHK(p, hipGetLastError());
    }
    if (nr) {
        pc_classes_kernel<<<(unsigned)((nr + 255) / 256), 256, 0, p->st>>>(p->nrows, p->psite.as<int32_t>(), p->porig.as<int64_t>(), K, T,
            dtab.as<PcTerm>(), dlo.as<double>(), dhi.as<double>(), c, dcnt.as<unsigned long long>());
        PCHK(p, hipGetLastError());
    }
    std::vector<unsigned long long> hc(ncnt);
    PCHK(p, hipMemcpyAsync(hc.data(), dcnt.p, ncnt * 8, hipMemcpyDeviceToHost, p->st));
    if (host && N) PCHK(p, hipMemcpyAsync(cls, c, N * 4, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipStreamSynchronize(p->st));
    for (size_t i = 0; i < ncnt; ++i) counts[i] = (int64_t)hc[i];
    return BH_OK;
}

int bh_posterior_scalar_export(bh_posterior *p, int set, int memspace, void *stream, int64_t ld, double *out)
{
    int rc;
    if (!p) return BH_EINVAL;
    if (p->S < 1) return pfail(p, BH_EINVAL, "no rows loaded (bh_posterior_load)");
    if (!p->has_rows) return pfail(p, BH_EINVAL, "the rows were loaded without bh_posterior_keep_rows");
    ScalarSet *ss;
    if ((rc = formed_set(p, set, "", &ss))) return rc;
    const int Q = ss->Q;
    if (ld < Q) return pfail(p, BH_EINVAL, "ld must be at least the set's columns");
    if (!out && p->ninput) return pfail(p, BH_EINVAL, "null argument");
    PCHK(p, hipSetDevice(p->device));
    const bool host = memspace != BH_DEVICE;
    p->st = (!host && stream) ? (hipStream_t)stream : (hipStream_t)bh_engine_stream(p->e);
    const size_t nr = (size_t)p->nrows, N = (size_t)p->ninput;
    if (!N) return BH_OK;
    Dev dout;
    if (host && (rc = alloc(p, dout, N * Q * 8))) return rc;   // (tight on the device; the copy back strides by ld)
    double *o = host ? dout.as<double>() : out;
    const int64_t old = host ? (int64_t)Q : ld;
    pc_export_fill_kernel<<<(unsigned)((N * Q + 255) / 256), 256, 0, p->st>>>(p->ninput, Q, old, o);
    PCHK(p, hipGetLastError());
    if (nr) {
        pc_export_kernel<<<(unsigned)((nr + 255) / 256), 256, 0, p->st>>>(p->nrows, p->porig.as<int64_t>(), Q, ss->val.as<double>(), old, o);
        PCHK(p, hipGetLastError());
    }
    if (host) PCHK(p, hipMemcpy2DAsync(out, (size_t)ld * 8, o, (size_t)Q * 8, (size_t)Q * 8, N, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipStreamSynchronize(p->st));
    return BH_OK;
}

} // extern "C"
