// bayhunter_amd/csrc/chain_diag_features_kernel.hip -- the structural features of the chains' recorded models as time-ordered series
// (include/bh_engine_chain_diag_features.h).
//
// The models are read where record="device" wrote them, [rows][C][2*ML]; the outputs are the tables [rows][K][ncols] that
// bh_chain_diag_series reads.  An element is one (row t, series k), k fastest.
//
// check kernel   : one lane per element.  The lane finds its chain (k, or sel[t][k] clamped into [0, C) and flagged), scans its row
//                  once and flags a value that is not finite and a row that is no model.  Nothing is written before the host has
//                  seen the flags.
// feature kernel : one lane per element, one wavefront per workgroup.  The lane counts its row's layers and walks the row once per
//                  feature with the walk of feature_rule.h -- the code bh_posterior_features runs on a loaded row, here with the
//                  depths formed on the way from the row's z --, at the parameters of its series' site, par[site[k]].  Consecutive
//                  lanes read rows ld_c apart (as rank_extract_kernel<.., true>); a row is an L1 / L2 hit after the first walk.
//                  A lane's ncols results lie ncols apart in the output, so they go through an LDS tile [ncols][65] (written
//                  [q][lane]: consecutive banks; read with a stride of 65 doubles: no conflict within a 32-lane half) and leave as
//                  consecutive addresses of the wavefront, as rs_fill_kernel's do.  With leading dimensions that leave gaps the
//                  address of every item is formed from its (t, k).
// missing kernel : one thread per (series, column) and block of rows counts the zeros of `present`; integer atomics.
// No private array, nothing indexed dynamically: no scratch.  -ffp-contract=off (Makefile) is the contract's.
#include "bh_hostkit.h"
#include "chain_tables.h"
#include "feature_rule.h"
#include "../../include/bh_engine_chain_diag_features.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#pragma clang fp contract(off)

#define CF_LANES 64      // elements of a workgroup of the feature kernel: one wavefront
#define CF_PITCH 65      // the LDS tile's row
#define CF_ROWS 256      // rows of a block of the missing kernel (more where the grid would not hold them)

namespace {

using namespace bhkit;

struct FeatArgs {
    const void *x;
    int64_t T, ld_t, ld_c;
    int ML, C, K;
    const int32_t *sel;   // null: series k reads chain k
    int64_t ld_sel;
};

// the chain that series k reads at row t -- clamped into [0, C) before it is an address, a clamped one flagged
__device__ __forceinline__ int chain_of(const FeatArgs &a, int64_t t, int k, int &bad)
{
    if (!a.sel) return k;
    const int c = a.sel[t * a.ld_sel + k];
    const int cc = min(max(c, 0), a.C - 1);
    if (cc != c) bad |= 4;
    return cc;
}

// the layers of a row [vs_1..vs_n, z_1..z_n, NaN..] of 2*ML values: a non-NaN value that is not finite sets bad |= 1, a row whose
// non-NaN values are not a non-empty prefix of even length sets bad |= 2 and has 0 layers (chain_diag_value.h's scan)
template <typename T> __device__ __forceinline__ int row_layers(const T *row, int ML, int &bad)
{
    const int W = 2 * ML;
    int cnt = 0, first = W;
    for (int i = 0; i < W; ++i) {
        const T v = row[i];
        const bool nan = v != v;
        cnt += nan ? 0 : 1;
        first = (nan && i < first) ? i : first;
        if (!nan && !(fabs((double)v) <= DBL_MAX)) bad |= 1;
    }
    if (cnt == 0 || cnt != first || (cnt & 1)) {
        bad |= 2;
        return 0;
    }
    return cnt / 2;
}

template <typename T> __global__ void __launch_bounds__(256) cf_check_kernel(FeatArgs a, int *flag)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.T * a.K) return;
    const int64_t t = e / a.K;
    const int k = (int)(e - t * a.K);
    int bad = 0;
    const int c = chain_of(a, t, k, bad);
    (void)row_layers((const T *)a.x + t * a.ld_t + (int64_t)c * a.ld_c, a.ML, bad);
    if (bad) atomicOr(flag, bad);
}

template <typename T>
__global__ void __launch_bounds__(CF_LANES) cf_features_kernel(FeatArgs a, int F, int ncols, const int32_t *__restrict__ kind,
                                                               const int32_t *__restrict__ col0, const double *__restrict__ par,
                                                               const int32_t *__restrict__ site, double *__restrict__ value,
                                                               float *__restrict__ present, int64_t ld_out_t, int64_t ld_out_k,
                                                               int packed)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *tv = (double *)smem;                                        // [ncols][CF_PITCH]
    float *tp = (float *)(smem + (size_t)ncols * CF_PITCH * sizeof(double));   // [ncols][CF_PITCH]
    const int lane = threadIdx.x;
    const int64_t NE = a.T * a.K, e0 = (int64_t)blockIdx.x * CF_LANES;
    const bool act = e0 + lane < NE;
    const int64_t e = act ? e0 + lane : e0;   // (a lane past the elements walks the block's first row again and stores nothing)
    const int64_t t = e / a.K;
    const int k = (int)(e - t * a.K);
    int bad = 0;
    const int c = chain_of(a, t, k, bad);
    const T *rp = (const T *)a.x + t * a.ld_t + (int64_t)c * a.ld_c;
    const StoreRow<T> row = {rp, row_layers(rp, a.ML, bad)};
    const int s = site[k];
    for (int f = 0; f < F; ++f) {
        const int c0 = col0[f];
        const double *pp = par + ((size_t)s * F + f) * 3;
        double va, vb;
        const bool two = feature_columns<T>(kind[f], row.n, row, pp[0], pp[1], pp[2], va, vb);
        tv[c0 * CF_PITCH + lane] = va == va ? va : 0.0;
        tp[c0 * CF_PITCH + lane] = va == va ? 1.0f : 0.0f;
        if (two) {   // (the kind is the wavefront's)
            tv[(c0 + 1) * CF_PITCH + lane] = vb == vb ? vb : 0.0;
            tp[(c0 + 1) * CF_PITCH + lane] = vb == vb ? 1.0f : 0.0f;
        }
    }
    __syncthreads();
    // the block's items (element el, column q), q fastest, 64 at a time: item i = el * ncols + q
    const int nel = (int)(NE - e0 < CF_LANES ? NE - e0 : CF_LANES);
    const int nitems = nel * ncols, dq = CF_LANES % ncols, de = CF_LANES / ncols;
    int el = lane / ncols, q = lane - el * ncols;
    for (int i = lane; i < nitems; i += CF_LANES) {
        int64_t at;
        if (packed) {
            at = e0 * ncols + i;
        } else {
            const int64_t ee = e0 + el, tt = ee / a.K;
            at = tt * ld_out_t + (ee - tt * a.K) * ld_out_k + q;
        }
        value[at] = tv[q * CF_PITCH + el];
        present[at] = tp[q * CF_PITCH + el];
        q += dq;
        el += de;
        if (q >= ncols) {
            q -= ncols;
            ++el;
        }
    }
}

// missing[k][q] += the rows t0 <= t < t0 + rows of series k that lack column q
__global__ void __launch_bounds__(256) cf_missing_kernel(int64_t T, int K, int ncols, int64_t rows, const float *__restrict__ present,
                                                         int64_t ld_out_t, int64_t ld_out_k, unsigned long long *missing)
{
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= (int64_t)K * ncols) return;
    const int k = (int)(w / ncols), q = (int)(w - (int64_t)k * ncols);
    const int64_t t0 = (int64_t)blockIdx.y * rows, t1 = t0 + rows < T ? t0 + rows : T;
    const float *p = present + (int64_t)k * ld_out_k + q;
    unsigned long long cnt = 0;
    for (int64_t t = t0; t < t1; ++t) cnt += p[t * ld_out_t] == 0.0f ? 1u : 0u;
    if (cnt) atomicAdd(&missing[w], cnt);
}

template <typename T>
int features_run(bh_engine *e, hipStream_t st, bool host, const FeatArgs &a, int F, int ncols, const int32_t *dkind, const int32_t *dcol0,
                 const double *dpar, const int32_t *dsite, double *value, float *present, int64_t ld_out_t, int64_t ld_out_k,
                 int64_t *missing)
{
    int rc;
    const int64_t NE = a.T * a.K;
    const size_t nmiss = (size_t)a.K * ncols;
    Buf dflag, dmiss, dval, dpres;
    if ((rc = alloc(e, dflag, 8)) || (rc = alloc(e, dmiss, nmiss * 8))) return rc;
    BH_CHK(e, hipMemsetAsync(dflag.p, 0, 8, st));
    cf_check_kernel<T><<<dim3((unsigned)((NE + 255) / 256)), 256, 0, st>>>(a, dflag.as<int>());
    BH_CHK(e, hipGetLastError());
    int flag = 0;
    BH_CHK(e, hipMemcpyAsync(&flag, dflag.p, 4, hipMemcpyDeviceToHost, st));
    BH_CHK(e, hipStreamSynchronize(st));
    if (flag & 4) return fail(e, BH_EINVAL, "a selection index is outside [0, C)");
    if (flag & 2) return fail(e, BH_EINVAL, "a model row's non-NaN values are not a non-empty prefix of even length");
    if (flag & 1) return fail(e, BH_EINVAL, "a value is not finite");
    // tables in host memory: formed packed on the device, copied, and laid out with the caller's leading dimensions
    double *dv = value;
    float *dp = present;
    int64_t lt = ld_out_t, lk = ld_out_k;
    if (host) {
        if ((rc = alloc(e, dval, (size_t)NE * ncols * 8)) || (rc = alloc(e, dpres, (size_t)NE * ncols * 4))) return rc;
        dv = dval.as<double>();
        dp = dpres.as<float>();
        lk = ncols;
        lt = (int64_t)a.K * ncols;
    }
    const int packed = (lk == ncols && lt == (int64_t)a.K * ncols) ? 1 : 0;
    BH_CHK(e, hipMemsetAsync(dmiss.p, 0, nmiss * 8, st));
    cf_features_kernel<T><<<dim3((unsigned)((NE + CF_LANES - 1) / CF_LANES)), CF_LANES, (size_t)ncols * CF_PITCH * 12, st>>>(
        a, F, ncols, dkind, dcol0, dpar, dsite, dv, dp, lt, lk, packed);
    BH_CHK(e, hipGetLastError());
    const int64_t rows = std::max<int64_t>(CF_ROWS, (a.T + 65534) / 65535);
    cf_missing_kernel<<<dim3((unsigned)((nmiss + 255) / 256), (unsigned)((a.T + rows - 1) / rows)), 256, 0, st>>>(
        a.T, a.K, ncols, rows, dp, lt, lk, dmiss.as<unsigned long long>());
    BH_CHK(e, hipGetLastError());
    std::vector<unsigned long long> hm(nmiss);
    std::vector<double> hv;
    std::vector<float> hp;
    BH_CHK(e, hipMemcpyAsync(hm.data(), dmiss.p, nmiss * 8, hipMemcpyDeviceToHost, st));
    if (host) {
        hv.resize((size_t)NE * ncols);
        hp.resize((size_t)NE * ncols);
        BH_CHK(e, hipMemcpyAsync(hv.data(), dv, hv.size() * 8, hipMemcpyDeviceToHost, st));
        BH_CHK(e, hipMemcpyAsync(hp.data(), dp, hp.size() * 4, hipMemcpyDeviceToHost, st));
    }
    BH_CHK(e, hipStreamSynchronize(st));
    for (size_t i = 0; i < nmiss; ++i) missing[i] = (int64_t)hm[i];
    if (host)
        for (int64_t t = 0; t < a.T; ++t)
            for (int k = 0; k < a.K; ++k) {
                const size_t from = ((size_t)t * (size_t)a.K + (size_t)k) * (size_t)ncols;
                const int64_t at = t * ld_out_t + (int64_t)k * ld_out_k;
                for (int q = 0; q < ncols; ++q) {
                    value[at + q] = hv[from + q];
                    present[at + q] = hp[from + q];
                }
            }
    return BH_OK;
}

} // namespace

extern "C" int bh_chain_diag_features(bh_engine *e, int memspace, void *stream, int elem_bytes, int64_t T, int C, int ML, int64_t ld_t,
                                      int64_t ld_c, const void *models, int K, const int32_t *sel, int64_t ld_sel, int nsites,
                                      const int32_t *site, int F, const int32_t *kind, const double *par, double *value, float *present,
                                      int64_t ld_out_t, int64_t ld_out_k, int64_t *missing)
{
    int rc;
    bh_chain_refusal no;
    if (!e) return BH_EINVAL;
    if (elem_bytes != 4 && elem_bytes != 8) return fail(e, BH_EINVAL, "the table must be float32 or float64");
    if (!models || !site || !value || !present || !missing) return fail(e, BH_EINVAL, "null argument");
    if (nsites < 1) return fail(e, BH_EINVAL, "nsites: at least one site");
    std::vector<int32_t> col0;
    std::string what;
    int ncols = 0;
    if ((rc = feature_table(F, kind, par, nsites, col0, ncols, what))) return fail(e, rc, what);
    if ((no = bh_chain_model_table(ML, 0, nullptr)).code) return fail(e, no.code, no.text);
    if ((no = bh_chain_table_span(T, C, 2 * (int64_t)ML, ld_t, ld_c)).code) return fail(e, no.code, no.text);
    if (sel) {
        if ((no = bh_chain_sel_span(T, K, 1, ld_sel)).code) return fail(e, no.code, no.text);
    } else if (K != C) {
        return fail(e, BH_EINVAL, "without a selection K must equal C: series k reads chain k");
    }
    if ((no = bh_chain_table_span(T, K, ncols, ld_out_t, ld_out_k)).code) return fail(e, BH_EINVAL, "bad leading dimensions of the outputs");
    if ((long double)T * (long double)K >= 68719476736.0L) return fail(e, BH_EINVAL, "T * K must stay below 2^36");
    if ((int64_t)K * ncols > (int64_t)INT_MAX) return fail(e, BH_EINVAL, "K * columns must stay below 2^31");
    for (int k = 0; k < K; ++k)
        if (site[k] < 0 || site[k] >= nsites) return fail(e, BH_EINVAL, "site[" + std::to_string(k) + "]: outside [0, nsites)");
    BH_CHK(e, hipSetDevice(bh_engine_device_internal(e)));
    const bool host = memspace != BH_DEVICE;
    hipStream_t st = call_stream(e, memspace, stream);
    Buf copy, csel, dkind, dcol0, dpar, dsite;
    FeatArgs a;
    a.sel = nullptr; a.ld_sel = ld_sel; a.C = C; a.K = K; a.T = T; a.ld_t = ld_t; a.ld_c = ld_c; a.ML = ML;
    const size_t span = (size_t)((T - 1) * ld_t + (int64_t)(C - 1) * ld_c + 2 * (int64_t)ML) * (size_t)elem_bytes;
    if ((rc = stage(e, st, memspace, models, span, copy, &a.x))) return rc;
    if (sel && (rc = stage(e, st, memspace, sel, (size_t)((T - 1) * ld_sel + K) * sizeof(int32_t), csel, &a.sel))) return rc;
    const std::vector<int32_t> hkind(kind, kind + F), hsite(site, site + K);
    const std::vector<double> hpar(par, par + (size_t)nsites * F * 3);
    if ((rc = upload(e, st, dkind, hkind)) || (rc = upload(e, st, dcol0, col0)) || (rc = upload(e, st, dpar, hpar)) ||
        (rc = upload(e, st, dsite, hsite)))
        return rc;
    rc = elem_bytes == 4 ? features_run<float>(e, st, host, a, F, ncols, dkind.as<int32_t>(), dcol0.as<int32_t>(), dpar.as<double>(),
                                               dsite.as<int32_t>(), value, present, ld_out_t, ld_out_k, missing)
                         : features_run<double>(e, st, host, a, F, ncols, dkind.as<int32_t>(), dcol0.as<int32_t>(), dpar.as<double>(),
                                                dsite.as<int32_t>(), value, present, ld_out_t, ld_out_k, missing);
    (void)hipStreamSynchronize(st);   // (the buffers and the host vectors go with this frame)
    return rc;
}
