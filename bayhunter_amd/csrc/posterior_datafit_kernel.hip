// bayhunter_amd/csrc/posterior_datafit_kernel.hip -- posterior data fits of many sites (include/bh_engine_posterior_datafit.h).
//
//   layers  : one lane per loaded row writes nlay, h, vp, vs, rho in the layout bh_evaluate_sites takes; no private array, the
//             mantle rule carried as one flag down the layers
//   best    : two passes of integer atomicMin per (site, chain): the ordered key of the misfit, then the input index over the rows
//             that hold that key (a third writes the winner's position among the loaded rows)
//   fill    : ymod [nb][ldy] -> val[q * nrows + r] through an LDS tile of 64 x 64 float64, rows 65 apart: a wavefront reads 64
//             consecutive q of a row (512 B) and writes 64 consecutive r of a column; the tile's ds_write_b64 are contiguous,
//             its ds_read_b64 go 130 dwords apart -- lanes 0..31 to the even banks 0..62 of 64, one 2-bank pair each: no conflict
//   quantiles : the radix select of posterior_select.h for R ranks in one read of the column per pass
// Chunks meet in integer atomics only, so the results are the same bits in every run, alone or among other sites.
// LDS: 33 280 B (fill: 4 workgroups of 256 lanes beside each other on a CU's 160 KiB), 8 KiB (the select of 8 ranks).  No kernel uses scratch
// (profiles/posterior_datafits_kernels.txt).  -ffp-contract=off (Makefile): rho's product is rounded before its sum.
#include "posterior_select.h"

#include <algorithm>
#include <cstring>

#define DF_THREADS 256
#define DF_TILE 64

using namespace bhpost;

namespace {

// one lane per row of [r0, r1): the layer rule (header)
template <typename T, typename V>
__global__ void __launch_bounds__(256) df_layers_kernel(int64_t r0, int64_t nb, int ML, const int32_t *pn, const int32_t *psite,
                                                        const int64_t *porig, const T *pvs, const T *pzd, const V *vpvs,
                                                        int64_t vstride, const double *mvs, const double *mvpvs, int32_t *nlay,
                                                        double *h, double *vp, double *vs, double *rho, int64_t sl, int32_t *site)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    const int64_t r = r0 + b;
    const int n = pn[r], s = psite[r];
    const T *rvs = pvs + r * ML, *rzd = pzd + r * ML;
    const T k = (T)vpvs[porig[r] * vstride];
    const bool rule = mvs && mvs[s] > 0.0;
    const T mv = rule ? (T)mvs[s] : (T)0, mk = rule ? (T)mvpvs[s] : (T)0;
    nlay[b] = n;
    site[b] = s;
    bool deep = false;
    double zprev = 0.0;
    for (int j = 0; j < ML; ++j) {
        double oh = 0.0, ovp = 0.0, ovs = 0.0, orho = 0.0;
        if (j < n) {
            const T v = rvs[j];
            deep = deep || (rule && v >= mv);
            const T p = v * (deep ? mk : k);
            const T pr = p * (T)0.32;
            const T d = pr + (T)0.77;
            if (j < n - 1) {
                const double zd = (double)rzd[j];
                oh = zd - zprev;
                zprev = zd;
            }
            ovp = (double)p;
            ovs = (double)v;
            orho = (double)d;
        }
        const int64_t o = (int64_t)j * sl + b;
        h[o] = oh;
        vp[o] = ovp;
        vs[o] = ovs;
        rho[o] = orho;
    }
}

struct BestArgs {
    int64_t nrows;
    const int32_t *psite;
    const int64_t *porig;
    const int32_t *chain;
    int64_t cstride;
    int nchains;
};

template <typename V>
__device__ __forceinline__ unsigned long long best_key(const V *misfit, int64_t mstride, int64_t i, bool *isnan)
{
    double m = (double)misfit[i * mstride];
    *isnan = m != m;
    m = m + 0.0;   // (-0.0 -> 0.0: numpy.argmin takes them as equal)
    return okey(m, false);
}

// pass 1: the least ordered key of every (site, chain); flag bit 0: a chain id out of range, bit 1: a NaN misfit
template <typename V>
__global__ void __launch_bounds__(256) df_best_key_kernel(BestArgs a, const V *misfit, int64_t mstride, unsigned long long *kmin,
                                                          int *flag)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.nrows) return;
    const int64_t i = a.porig[r];
    const int c = a.chain[i * a.cstride];
    if (c < 0 || c >= a.nchains) { atomicOr(flag, 1); return; }
    bool isnan;
    const unsigned long long k = best_key(misfit, mstride, i, &isnan);
    if (isnan) { atomicOr(flag, 2); return; }
    atomicMin(&kmin[(size_t)a.psite[r] * a.nchains + c], k);
}

// pass 2: the least input index among the rows that hold the least key
template <typename V>
__global__ void __launch_bounds__(256) df_best_idx_kernel(BestArgs a, const V *misfit, int64_t mstride,
                                                          const unsigned long long *kmin, unsigned long long *imin)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.nrows) return;
    const int64_t i = a.porig[r];
    const int c = a.chain[i * a.cstride];
    if (c < 0 || c >= a.nchains) return;
    bool isnan;
    const unsigned long long k = best_key(misfit, mstride, i, &isnan);
    const size_t cell = (size_t)a.psite[r] * a.nchains + c;
    if (!isnan && k == kmin[cell]) atomicMin(&imin[cell], (unsigned long long)i);
}

// pass 3: the winner's position among the loaded rows (one row per cell: a plain store)
__global__ void __launch_bounds__(256) df_best_pos_kernel(BestArgs a, const unsigned long long *imin, long long *pos)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.nrows) return;
    const int64_t i = a.porig[r];
    const int c = a.chain[i * a.cstride];
    if (c < 0 || c >= a.nchains) return;
    const size_t cell = (size_t)a.psite[r] * a.nchains + c;
    if (imin[cell] == (unsigned long long)i) pos[cell] = (long long)r;
}

// workgroup (x: 64 rows of the batch, y: 64 columns): ymod -> the DATA set's columns, masked (header)
__global__ void __launch_bounds__(DF_THREADS) df_fill_kernel(int64_t r0, int64_t nb, int ldy, int64_t nrows, const double *ymod,
                                                             const int32_t *err, const int32_t *psite, int nt,
                                                             const int32_t *ncol, const int32_t *colt, const int32_t *colj,
                                                             double *val, unsigned long long *failed)
{
    __shared__ double tile[DF_TILE][DF_TILE + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t rb = (int64_t)blockIdx.x * DF_TILE;
    const int qb = blockIdx.y * DF_TILE;
    const int q = qb + lane;
    const int t = q < ldy ? colt[q] : 0, j = q < ldy ? colj[q] : 0;
    for (int i = 0; i < DF_TILE / 4; ++i) {
        const int lr = w * (DF_TILE / 4) + i;
        const int64_t b = rb + lr;   // (uniform over the wavefront)
        double v = qnan();
        if (b < nb && q < ldy && err[b] == 0 && j < ncol[(size_t)psite[r0 + b] * nt + t]) v = ymod[b * ldy + q];
        tile[lr][lane] = v;
    }
    __syncthreads();
    const int64_t b = rb + lane;
    for (int i = 0; i < DF_TILE / 4; ++i) {
        const int lq = w * (DF_TILE / 4) + i;
        if (b < nb && qb + lq < ldy) val[(int64_t)(qb + lq) * nrows + r0 + b] = tile[lane][lq];
    }
    if (blockIdx.y == 0 && w == 0) {   // (a whole wavefront: agg_add is called by all its lanes)
        const bool bad = b < nb && err[b] != 0;
        agg_add(failed, bad ? psite[r0 + b] : 0, bad);
    }
}

// one lane per (row, column) of the gather
__global__ void __launch_bounds__(256) df_gather_kernel(int64_t n, int Q, int64_t nrows, const double *val, const int64_t *pos,
                                                        double *out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * Q) return;
    out[i] = val[(i % Q) * nrows + pos[i / Q]];
}

// ---- host side ---------------------------------------------------------------------------------------------------

int need_rows(bh_posterior *p)
{
    if (p->S < 1) return pfail(p, BH_EINVAL, "no rows loaded (bh_posterior_load)");
    if (!p->has_rows) return pfail(p, BH_EINVAL, "the rows were loaded without bh_posterior_keep_rows");
    return BH_OK;
}

void use_stream(bh_posterior *p, bool host, void *stream)
{
    p->st = (!host && stream) ? (hipStream_t)stream : (hipStream_t)bh_engine_stream(p->e);
}

// a host array of one value per input row, `stride` elements apart, to the device (dv); *out: the device pointer
int to_device(bh_posterior *p, Dev &dv, bool host, const void *v, int64_t stride, size_t eb, const void **out)
{
    int rc;
    *out = v;
    if (!host || !p->ninput) return BH_OK;
    const size_t n = (size_t)((p->ninput - 1) * stride + 1);
    if ((rc = alloc(p, dv, n * eb))) return rc;
    PCHK(p, hipMemcpyAsync(dv.p, v, n * eb, hipMemcpyHostToDevice, p->st));
    *out = dv.p;
    return BH_OK;
}

} // namespace

extern "C" {

int bh_posterior_layers(bh_posterior *p, int64_t r0, int64_t r1, int memspace, void *stream, int vpvs_elem, int64_t vpvs_stride,
                        const void *vpvs, const double *mantle_vs, const double *mantle_vpvs, int32_t *nlay, double *h,
                        double *vp, double *vs, double *rho, int64_t stride_l, int32_t *site)
{
    int rc;
    if (!p) return BH_EINVAL;
    if ((rc = need_rows(p))) return rc;
    if (r0 < 0 || r1 < r0 || r1 > p->nrows) return pfail(p, BH_EINVAL, "rows [r0, r1) are not among the loaded rows");
    if (vpvs_elem != 4 && vpvs_elem != 8) return pfail(p, BH_EINVAL, "vpvs must be float32 or float64");
    if (vpvs_stride < 1 || (!vpvs && p->ninput)) return pfail(p, BH_EINVAL, "bad vpvs stride or null vpvs");
    if (!nlay || !h || !vp || !vs || !rho || !site) return pfail(p, BH_EINVAL, "null argument");
    if (stride_l < r1 - r0) return pfail(p, BH_EINVAL, "stride_l is below the number of rows");
    if ((mantle_vs == nullptr) != (mantle_vpvs == nullptr)) return pfail(p, BH_EINVAL, "mantle_vs and mantle_vpvs go together");
    PCHK(p, hipSetDevice(p->device));
    const bool host = memspace != BH_DEVICE;
    use_stream(p, host, stream);
    const int64_t nb = r1 - r0;
    if (!nb) return BH_OK;
    Dev dv;
    const void *v;
    if ((rc = to_device(p, dv, host, vpvs, vpvs_stride, (size_t)vpvs_elem, &v))) return rc;
    const double *mvs = nullptr, *mk = nullptr;
    if (mantle_vs) {   // the table stays in the handle: uploaded again only where it differs from the last call's
        const size_t S = (size_t)p->S;
        std::vector<double> tab(2 * S);
        std::memcpy(tab.data(), mantle_vs, S * 8);
        std::memcpy(tab.data() + S, mantle_vpvs, S * 8);
        if (!p->mantle_tab.p || p->mantle_host.size() != tab.size() || std::memcmp(p->mantle_host.data(), tab.data(), tab.size() * 8)) {
            PCHK(p, hipStreamSynchronize(p->st));   // (no launch still reads the table that goes)
            p->mantle_host.clear();
            if ((rc = alloc(p, p->mantle_tab, S * 16))) return rc;
            PCHK(p, hipMemcpy(p->mantle_tab.p, tab.data(), S * 16, hipMemcpyHostToDevice));
            p->mantle_host = tab;
        }
        mvs = p->mantle_tab.as<double>();
        mk = mvs + S;
    }
    const unsigned nblk = (unsigned)((nb + 255) / 256);
#define DF_LAYERS(T, V)                                                                                                       \
    df_layers_kernel<T, V><<<nblk, 256, 0, p->st>>>(r0, nb, p->ML, p->pn.as<int32_t>(), p->psite.as<int32_t>(), p->porig.as<int64_t>(), \
                                                    p->pvs.as<T>(), p->pzd.as<T>(), (const V *)v, vpvs_stride, mvs, mk, nlay, h, vp, vs, \
                                                    rho, stride_l, site)
    if (p->elem == 4 && vpvs_elem == 4) DF_LAYERS(float, float);
    else if (p->elem == 4) DF_LAYERS(float, double);
    else if (vpvs_elem == 4) DF_LAYERS(double, float);
    else DF_LAYERS(double, double);
#undef DF_LAYERS
    PCHK(p, hipGetLastError());
    if (dv.p) PCHK(p, hipStreamSynchronize(p->st));   // (the copy of a host vpvs is freed on return)
    return BH_OK;
}

int bh_posterior_best(bh_posterior *p, int nchains, int memspace, void *stream, const int32_t *chain, int64_t chain_stride,
                      int misfit_elem, const void *misfit, int64_t misfit_stride, int64_t *best, int64_t *pos)
{
    int rc;
    if (!p) return BH_EINVAL;
    if ((rc = need_rows(p))) return rc;
    if (nchains < 1 || (int64_t)p->S * nchains > (1 << 24)) return pfail(p, BH_EINVAL, "nchains: 1 .. 2^24 / nsites");
    if (misfit_elem != 4 && misfit_elem != 8) return pfail(p, BH_EINVAL, "misfits must be float32 or float64");
    if (chain_stride < 1 || misfit_stride < 1 || !best || ((!chain || !misfit) && p->ninput))
        return pfail(p, BH_EINVAL, "bad stride or null argument");
    const bool host = memspace != BH_DEVICE;
    if (host)
        for (int64_t i = 0; i < p->ninput; ++i)
            if (chain[i * chain_stride] < 0 || chain[i * chain_stride] >= nchains) return pfail(p, BH_EINVAL, "chain id out of range");
    PCHK(p, hipSetDevice(p->device));
    use_stream(p, host, stream);
    const size_t ncell = (size_t)p->S * nchains;
    Dev dc, dm, dk, di, dp, df;
    const void *c, *m;
    if ((rc = to_device(p, dc, host, chain, chain_stride, 4, &c)) || (rc = to_device(p, dm, host, misfit, misfit_stride, (size_t)misfit_elem, &m)))
        return rc;
    if ((rc = alloc(p, dk, ncell * 8)) || (rc = alloc(p, di, ncell * 8)) || (rc = alloc(p, dp, ncell * 8)) || (rc = alloc(p, df, 4))) return rc;
    PCHK(p, hipMemsetAsync(dk.p, 0xff, ncell * 8, p->st));
    PCHK(p, hipMemsetAsync(di.p, 0xff, ncell * 8, p->st));
    PCHK(p, hipMemsetAsync(dp.p, 0xff, ncell * 8, p->st));   // (-1)
    PCHK(p, hipMemsetAsync(df.p, 0, 4, p->st));
    const BestArgs a{p->nrows, p->psite.as<int32_t>(), p->porig.as<int64_t>(), (const int32_t *)c, chain_stride, nchains};
    const unsigned nblk = (unsigned)((p->nrows + 255) / 256);
    int flag = 0;
    if (p->nrows) {
        if (misfit_elem == 4) df_best_key_kernel<float><<<nblk, 256, 0, p->st>>>(a, (const float *)m, misfit_stride, dk.as<unsigned long long>(), df.as<int>());
        else df_best_key_kernel<double><<<nblk, 256, 0, p->st>>>(a, (const double *)m, misfit_stride, dk.as<unsigned long long>(), df.as<int>());
        PCHK(p, hipGetLastError());
        PCHK(p, hipMemcpyAsync(&flag, df.p, 4, hipMemcpyDeviceToHost, p->st));
        PCHK(p, hipStreamSynchronize(p->st));
        if (flag & 1) return pfail(p, BH_EINVAL, "chain id out of range");
        if (flag & 2) return pfail(p, BH_EINVAL, "a misfit is NaN");
        if (misfit_elem == 4)
            df_best_idx_kernel<float><<<nblk, 256, 0, p->st>>>(a, (const float *)m, misfit_stride, dk.as<unsigned long long>(), di.as<unsigned long long>());
        else
            df_best_idx_kernel<double><<<nblk, 256, 0, p->st>>>(a, (const double *)m, misfit_stride, dk.as<unsigned long long>(), di.as<unsigned long long>());
        df_best_pos_kernel<<<nblk, 256, 0, p->st>>>(a, di.as<unsigned long long>(), dp.as<long long>());
        PCHK(p, hipGetLastError());
    }
    PCHK(p, hipMemcpyAsync(best, di.p, ncell * 8, hipMemcpyDeviceToHost, p->st));   // (~0 = -1: no row)
    if (pos) PCHK(p, hipMemcpyAsync(pos, dp.p, ncell * 8, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipStreamSynchronize(p->st));
    return BH_OK;
}

int bh_posterior_data_fill(bh_posterior *p, void *stream, int64_t r0, int64_t nb, int ldy, const double *ymod, const int32_t *err,
                           int nt, const int32_t *ncol, int64_t *failed)
{
    int rc;
    if (!p) return BH_EINVAL;
    if ((rc = need_rows(p))) return rc;
    if (ldy < 1 || ldy > BH_DATAFIT_MAXCOLS) return pfail(p, BH_EINVAL, "columns: 1..BH_DATAFIT_MAXCOLS");
    if (nt < 1 || nt > BH_MAX_TARGETS || !ncol) return pfail(p, BH_EINVAL, "bad target count or null ncol");
    if (nb < 0 || r0 < 0 || r0 + nb > p->nrows || (nb && (!ymod || !err))) return pfail(p, BH_EINVAL, "rows [r0, r0 + nb) are not among the loaded rows");
    if (r0 != 0 && (p->data_filled != r0 || p->data_ldy != ldy))
        return pfail(p, BH_EINVAL, "bh_posterior_data_fill calls go in order from r0 = 0 with one ldy");
    // the column blocks: target t's is as wide as its largest count
    std::vector<int32_t> colt(ldy), colj(ldy);
    int64_t off = 0;
    for (int t = 0; t < nt; ++t) {
        int cap = 0;
        for (int s = 0; s < p->S; ++s) {
            const int c = ncol[(size_t)s * nt + t];
            if (c < 0) return pfail(p, BH_EINVAL, "a negative sample count");
            cap = std::max(cap, c);
        }
        if (off + cap > ldy) return pfail(p, BH_EINVAL, "the targets' column blocks do not add up to ldy");
        for (int j = 0; j < cap; ++j) { colt[off + j] = t; colj[off + j] = j; }
        off += cap;
    }
    if (off != ldy) return pfail(p, BH_EINVAL, "the targets' column blocks do not add up to ldy");
    PCHK(p, hipSetDevice(p->device));
    p->st = stream ? (hipStream_t)stream : (hipStream_t)bh_engine_stream(p->e);
    ScalarSet &ss = p->sets[set_slot(BH_SCALARS_DATA)];
    const size_t S = (size_t)p->S;
    if (r0 == 0) {
        ss.drop();
        p->data_filled = -1;
        if ((rc = alloc(p, ss.val, (size_t)p->nrows * ldy * 8)) || (rc = alloc(p, p->data_failed, S * 8))) return rc;
        PCHK(p, hipMemsetAsync(p->data_failed.p, 0, S * 8, p->st));
        // the tables of the whole fill: ncol, and every column's target and index in it
        std::vector<int32_t> tab(S * nt + 2 * (size_t)ldy);
        std::memcpy(tab.data(), ncol, S * nt * 4);
        std::memcpy(tab.data() + S * nt, colt.data(), (size_t)ldy * 4);
        std::memcpy(tab.data() + S * nt + ldy, colj.data(), (size_t)ldy * 4);
        if ((rc = alloc(p, p->data_tab, tab.size() * 4))) return rc;
        PCHK(p, hipMemcpy(p->data_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
        p->data_ncol.assign(ncol, ncol + S * nt);
        p->data_ldy = ldy;
        p->data_filled = 0;
    } else if (p->data_ncol.size() != S * nt || std::memcmp(p->data_ncol.data(), ncol, S * nt * 4)) {
        return pfail(p, BH_EINVAL, "ncol differs from the table of the call that started the fill");
    }
    if (nb) {
        const int32_t *tab = p->data_tab.as<int32_t>();
        const dim3 grid((unsigned)((nb + DF_TILE - 1) / DF_TILE), (unsigned)((ldy + DF_TILE - 1) / DF_TILE));
        df_fill_kernel<<<grid, DF_THREADS, 0, p->st>>>(r0, nb, ldy, p->nrows, ymod, err, p->psite.as<int32_t>(), nt, tab, tab + S * nt,
                                                       tab + S * nt + ldy, ss.val.as<double>(), p->data_failed.as<unsigned long long>());
        PCHK(p, hipGetLastError());   // (asynchronous: ymod and err may be written again on the same stream)
    }
    p->data_filled = r0 + nb;
    if (p->data_filled == p->nrows) {
        std::vector<unsigned long long> hf(S);
        PCHK(p, hipMemcpyAsync(hf.data(), p->data_failed.p, S * 8, hipMemcpyDeviceToHost, p->st));
        PCHK(p, hipStreamSynchronize(p->st));
        if (failed)
            for (size_t s = 0; s < S; ++s) failed[s] = (int64_t)hf[s];
        ss.Q = ldy;
        p->data_filled = -1;
    }
    return BH_OK;
}

int bh_posterior_scalar_quantiles(bh_posterior *p, int set, int R, const uint32_t *rank, uint64_t *lower, uint64_t *upper)
{
    int rc;
    if (!p) return BH_EINVAL;
    ScalarSet *ss;
    if ((rc = get_set(p, set, &ss))) return rc;
    if (R < 1 || R > SELECT_MAXR) return pfail(p, BH_EINVAL, "ranks per column: 1..BH_QUANTILES_MAXRANKS");
    if (!rank || !lower || !upper) return pfail(p, BH_EINVAL, "null argument");
    const int Q = ss->Q;
    const size_t ncol = (size_t)p->S * Q;
    if (ss->count.size() != ncol || ss->nf.size() != (size_t)Q)
        return pfail(p, BH_EINVAL, "bh_posterior_scalar_stats has not run on the set since it was formed");
    for (size_t c = 0; c < ncol; ++c)
        for (int r = 0; r < R; ++r)
            if ((int64_t)rank[c * R + r] >= std::max<int64_t>(ss->count[c], 1)) return pfail(p, BH_EINVAL, "a rank is not below its column's count");
    PCHK(p, hipSetDevice(p->device));
    std::vector<int> kb(Q);
    for (int q = 0; q < Q; ++q) kb[q] = ss->nf[q] ? 64 : 32;
    return select_ranks(p, ncol, R, rank, ss->count.data(), kb, true, SetSelect{p, set_args(p, ss)}, lower, upper, 1);
}

int bh_posterior_scalar_gather(bh_posterior *p, int set, int64_t n, const int64_t *pos, double *out)
{
    int rc;
    if (!p) return BH_EINVAL;
    ScalarSet *ss;
    if ((rc = get_set(p, set, &ss))) return rc;
    if (n < 0 || (n && (!pos || !out))) return pfail(p, BH_EINVAL, "null argument");
    for (int64_t i = 0; i < n; ++i)
        if (pos[i] < 0 || pos[i] >= p->nrows) return pfail(p, BH_EINVAL, "a position is not among the loaded rows");
    if (!n) return BH_OK;
    PCHK(p, hipSetDevice(p->device));
    Dev dp, dout;
    const size_t tot = (size_t)n * ss->Q;
    if ((rc = alloc(p, dp, (size_t)n * 8)) || (rc = alloc(p, dout, tot * 8))) return rc;
    PCHK(p, hipMemcpyAsync(dp.p, pos, (size_t)n * 8, hipMemcpyHostToDevice, p->st));
    df_gather_kernel<<<(unsigned)((tot + 255) / 256), 256, 0, p->st>>>(n, ss->Q, p->nrows, ss->val.as<double>(), dp.as<int64_t>(), dout.as<double>());
    PCHK(p, hipGetLastError());
    PCHK(p, hipMemcpyAsync(out, dout.p, tot * 8, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipStreamSynchronize(p->st));
    return BH_OK;
}

} // extern "C"
