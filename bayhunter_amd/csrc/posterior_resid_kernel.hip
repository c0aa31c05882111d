// bayhunter_amd/csrc/posterior_resid_kernel.hip -- posterior residuals of many sites (include/bh_engine_posterior_resid.h).
//
//   fill : a workgroup takes 64 rows of the batch and one target slot, each of its 4 wavefronts 16 of the rows one after the other.
//          The wavefront's lanes are the 64 strands of the header's sums: lane j holds u_i of the current 64 samples and of the next
//          64, and u_{i+l} (l <= 32) comes by ONE lane shuffle per lag -- lane j reads lane (j + l) & 63 of the value "next where
//          lane < l, else current".  The butterfly s_j + s_{j xor w} is __shfl_xor, after which every lane holds every sum; lane q
//          forms column q.  No sample is read twice and nothing is staged: n is bounded by BH_DATAFIT_MAXCOLS only.
//          The 5 + L columns of the 64 rows go through an LDS tile [37][65] so that a wavefront writes 64 consecutive rows of a
//          column (val[q * nrows + r]); the tile's writes are 130 dwords apart (37 lanes at most: 2- to 3-way on ds_write's 32
//          banks), its reads contiguous.
// Rows meet nowhere but in the integer count of the failed ones: the same bits in every run, alone or among other sites, for any
// split into batches.  LDS 19 240 B; no scratch (`make resources`).  -ffp-contract=off (Makefile) and the pragma below: every
// product of the header is rounded before it is added.
#include "posterior_select.h"
#include "../../include/bh_engine_posterior_resid.h"

#include <algorithm>
#include <cstring>

#pragma clang fp contract(off)

#define RS_THREADS 256
#define RS_TILE 64
#define RS_MAXQ (BH_RESID_FIXED + BH_RESID_MAXLAG)

using namespace bhpost;

namespace {

struct ResidArgs {
    int64_t r0, nb, nrows;
    int ldy, nt, L;
    const double *ymod;
    const int32_t *err, *psite;
    const int64_t *porig;
    const int32_t *ncol, *toff;   // [S][nt]; [nt]: slot t's first column
    const double *yobs, *g;       // [S][ldy]; g may be null (1.0)
    int64_t noise_ld;
    double *val;
    unsigned long long *failed;
};

// the butterfly of the header: every lane ends with s_0
__device__ __forceinline__ double strand_sum(double v)
{
    for (int w = 32; w; w >>= 1) v = v + __shfl_xor(v, w);
    return v;
}

// workgroup (x: 64 rows of the batch, y: the slot)
template <typename V>
__global__ void __launch_bounds__(RS_THREADS) rs_fill_kernel(ResidArgs a, const V *noise)
{
    __shared__ double tile[RS_MAXQ][RS_TILE + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t rb = (int64_t)blockIdx.x * RS_TILE;
    const int t = blockIdx.y, L = a.L, QS = BH_RESID_FIXED + L;
    const int c0 = a.toff[t];
    for (int k = 0; k < RS_TILE / 4; ++k) {
        const int lr = w * (RS_TILE / 4) + k;
        const int64_t b = rb + lr;   // (uniform over the wavefront, as everything that branches below)
        if (b >= a.nb) break;
        const int64_t r = a.r0 + b;
        const int s = a.psite[r];
        const int n = a.ncol[(size_t)s * a.nt + t];
        double res = qnan();
        if (a.err[b] == 0 && n > 0) {
            const double *ym = a.ymod + b * a.ldy + c0, *yo = a.yobs + (int64_t)s * a.ldy + c0;
            const double *gg = a.g ? a.g + (int64_t)s * a.ldy + c0 : nullptr;
            double sb = 0.0, se = 0.0, acc[BH_RESID_MAXLAG + 1];
#pragma unroll
            for (int l = 0; l <= BH_RESID_MAXLAG; ++l) acc[l] = 0.0;
            double ec = 0.0, uc = 0.0;
            if (lane < n) {
                ec = ym[lane] - yo[lane];
                uc = gg ? ec * gg[lane] : ec;
            }
            for (int base = 0; base < n; base += 64) {
                const int i = base + lane, in = i + 64;
                double en = 0.0, un = 0.0;
                if (in < n) {
                    en = ym[in] - yo[in];
                    un = gg ? en * gg[in] : en;
                }
                if (i < n) {
                    sb = sb + ec;
                    se = se + ec * ec;
                    acc[0] = acc[0] + uc * uc;
                }
#pragma unroll
                for (int l = 1; l <= BH_RESID_MAXLAG; ++l) {
                    if (l <= L) {   // (no break: the loop unrolls and acc stays in registers)
                        const double v = __shfl(lane < l ? un : uc, (lane + l) & 63);   // u_{i+l}
                        if (i + l < n) acc[l] = acc[l] + uc * v;
                    }
                }
                ec = en;
                uc = un;
            }
            sb = strand_sum(sb);
            se = strand_sum(se);
            const double a0 = strand_sum(acc[0]);
            const double dn = (double)n;
            const V *nz = noise + a.porig[r] * a.noise_ld + 2 * t;
            const double corr = (double)nz[0], sigma = (double)nz[1];
            const bool quot = a0 != 0.0;
            double acf1 = qnan();
#pragma unroll
            for (int l = 1; l <= BH_RESID_MAXLAG; ++l) {
                if (l <= L) {
                    const double al = strand_sum(acc[l]);
                    const double q = (quot && l < n) ? al / a0 : qnan();
                    if (l == 1) acf1 = q;
                    if (lane == BH_RESID_FIXED + l - 1) res = q;
                }
            }
            if (lane == 0) res = sb / dn;
            if (lane == 1) res = sqrt(se / dn);
            if (lane == 2) res = sqrt(a0 / dn) / sigma;
            if (lane == 3) res = corr;
            if (lane == 4) res = acf1 - corr;
            if (!(fabs(res) <= 1.7976931348623157e308)) res = qnan();   // (nothing non-finite but this NaN is ever written)
        }
        if (lane < QS) tile[lane][lr] = res;
    }
    __syncthreads();
    const int64_t b = rb + lane;
    if (b < a.nb)
        for (int q = w; q < QS; q += RS_THREADS / 64) a.val[((int64_t)t * QS + q) * a.nrows + a.r0 + b] = tile[q][lane];
    if (t == 0 && w == 0) {   // (a whole wavefront: agg_add is called by all its lanes)
        const bool bad = b < a.nb && a.err[b] != 0;
        agg_add(a.failed, bad ? a.psite[a.r0 + b] : 0, bad);
    }
}

// a refusal ends the fill under way and leaves the set unformed
int refuse(bh_posterior *p, const char *what)
{
    p->sets[set_slot(BH_SCALARS_RESID)].drop();
    p->resid_filled = -1;
    return pfail(p, BH_EINVAL, std::string("bh_posterior_resid_fill: ") + what);
}

} // namespace

extern "C" {

int bh_posterior_resid_fill(bh_posterior *p, void *stream, int64_t r0, int64_t nb, int ldy, const double *ymod, const int32_t *err,
                            int nt, const int32_t *ncol, int L, const double *yobs, const double *g, int noise_memspace,
                            int noise_elem, int64_t noise_ld, const void *noise, int64_t *failed)
{
    int rc;
    if (!p) return BH_EINVAL;
    if (p->S < 1) return refuse(p, "no rows loaded (bh_posterior_load)");
    if (!p->has_rows) return refuse(p, "the rows were loaded without bh_posterior_keep_rows");
    if (L < 1 || L > BH_RESID_MAXLAG) return refuse(p, "lags: 1..BH_RESID_MAXLAG");
    if (ldy < 1 || ldy > BH_DATAFIT_MAXCOLS) return refuse(p, "columns of the synthetics: 1..BH_DATAFIT_MAXCOLS");
    if (nt < 1 || nt > BH_MAX_TARGETS || !ncol || !yobs) return refuse(p, "bad target count, null ncol or null yobs");
    const int QS = BH_RESID_FIXED + L, Q = nt * QS;
    if (Q > BH_DATAFIT_MAXCOLS) return refuse(p, "nt * (BH_RESID_FIXED + L) columns: at most BH_DATAFIT_MAXCOLS");
    if (noise_elem != 4 && noise_elem != 8) return refuse(p, "noise must be float32 or float64");
    if (noise_ld < 2 * (int64_t)nt || (!noise && p->ninput)) return refuse(p, "noise_ld below 2 * nt, or null noise");
    if (nb < 0 || r0 < 0 || r0 + nb > p->nrows || (nb && (!ymod || !err))) return refuse(p, "rows [r0, r0 + nb) are not among the loaded rows");
    const bool nhost = noise_memspace != BH_DEVICE;
    if (r0 != 0 && (p->resid_filled != r0 || p->resid_ldy != ldy || p->resid_nt != nt || p->resid_L != L))
        return refuse(p, "calls go in order from r0 = 0 with one ldy, nt and L");
    // the column blocks: target t's is as wide as its largest count
    const size_t S = (size_t)p->S;
    std::vector<int32_t> tab(S * nt + nt);
    int64_t off = 0;
    for (int t = 0; t < nt; ++t) {
        int cap = 0;
        for (size_t s = 0; s < S; ++s) {
            const int c = ncol[s * nt + t];
            if (c < 0) return refuse(p, "a negative sample count");
            cap = std::max(cap, c);
        }
        tab[S * nt + t] = (int32_t)off;
        off += cap;
        if (off > ldy) return refuse(p, "the targets' column blocks do not add up to ldy");
    }
    if (off != ldy) return refuse(p, "the targets' column blocks do not add up to ldy");
    std::memcpy(tab.data(), ncol, S * nt * 4);
    const size_t nobs = S * (size_t)ldy;
    if (r0 != 0) {
        if (p->resid_ncol.size() != S * nt || std::memcmp(p->resid_ncol.data(), ncol, S * nt * 4))
            return refuse(p, "ncol differs from the table of the call that started the fill");
        if (p->resid_g != (g != nullptr) || p->resid_host.size() != nobs * (g ? 2 : 1) || std::memcmp(p->resid_host.data(), yobs, nobs * 8) ||
            (g && std::memcmp(p->resid_host.data() + nobs, g, nobs * 8)))
            return refuse(p, "yobs or g differs from the table of the call that started the fill");
        if (p->resid_nmem != (nhost ? BH_HOST : BH_DEVICE) || p->resid_nelem != noise_elem || p->resid_nld != noise_ld)
            return refuse(p, "the noise table's memspace, element size or noise_ld differs from the call that started the fill");
    }
    PCHK(p, hipSetDevice(p->device));
    p->st = stream ? (hipStream_t)stream : (hipStream_t)bh_engine_stream(p->e);
    ScalarSet &ss = p->sets[set_slot(BH_SCALARS_RESID)];
    if (r0 == 0) {
        ss.drop();
        p->resid_filled = -1;
        if ((rc = alloc(p, ss.val, (size_t)p->nrows * Q * 8)) || (rc = alloc(p, p->resid_failed, S * 8))) return rc;
        PCHK(p, hipMemsetAsync(p->resid_failed.p, 0, S * 8, p->st));
        std::vector<double> obs(nobs * (g ? 2 : 1));
        std::memcpy(obs.data(), yobs, nobs * 8);
        if (g) std::memcpy(obs.data() + nobs, g, nobs * 8);
        if ((rc = alloc(p, p->resid_tab, tab.size() * 4)) || (rc = alloc(p, p->resid_obs, obs.size() * 8))) return rc;
        PCHK(p, hipMemcpy(p->resid_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
        PCHK(p, hipMemcpy(p->resid_obs.p, obs.data(), obs.size() * 8, hipMemcpyHostToDevice));
        if (nhost && p->ninput) {   // the host noise table, up to the last value a row can be asked for
            const size_t bytes = ((size_t)(p->ninput - 1) * noise_ld + 2 * (size_t)nt) * noise_elem;
            if ((rc = alloc(p, p->resid_noise, bytes))) return rc;
            PCHK(p, hipMemcpy(p->resid_noise.p, noise, bytes, hipMemcpyHostToDevice));
        }
        p->resid_ncol.assign(ncol, ncol + S * nt);
        p->resid_host.swap(obs);
        p->resid_g = g != nullptr;
        p->resid_nmem = nhost ? BH_HOST : BH_DEVICE;
        p->resid_nelem = noise_elem;
        p->resid_nld = noise_ld;
        p->resid_ldy = ldy;
        p->resid_nt = nt;
        p->resid_L = L;
        p->resid_filled = 0;
    }
    if (nb) {
        const int32_t *dt = p->resid_tab.as<int32_t>();
        const double *dobs = p->resid_obs.as<double>();
        const void *dn = nhost ? p->resid_noise.p : noise;
        const ResidArgs a{r0, nb, p->nrows, ldy, nt, L, ymod, err, p->psite.as<int32_t>(), p->porig.as<int64_t>(), dt, dt + S * nt,
                          dobs, g ? dobs + nobs : nullptr, noise_ld, ss.val.as<double>(), p->resid_failed.as<unsigned long long>()};
        const dim3 grid((unsigned)((nb + RS_TILE - 1) / RS_TILE), (unsigned)nt);
        if (noise_elem == 4) rs_fill_kernel<float><<<grid, RS_THREADS, 0, p->st>>>(a, (const float *)dn);
        else rs_fill_kernel<double><<<grid, RS_THREADS, 0, p->st>>>(a, (const double *)dn);
        PCHK(p, hipGetLastError());   // (asynchronous: ymod and err may be written again on the same stream)
    }
    p->resid_filled = r0 + nb;
    if (p->resid_filled == p->nrows) {
        std::vector<unsigned long long> hf(S);
        PCHK(p, hipMemcpyAsync(hf.data(), p->resid_failed.p, S * 8, hipMemcpyDeviceToHost, p->st));
        PCHK(p, hipStreamSynchronize(p->st));
        if (failed)
            for (size_t s = 0; s < S; ++s) failed[s] = (int64_t)hf[s];
        ss.Q = Q;
        p->resid_filled = -1;
    }
    return BH_OK;
}

} // extern "C"
