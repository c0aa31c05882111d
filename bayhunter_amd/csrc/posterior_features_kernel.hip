// bayhunter_amd/csrc/posterior_features_kernel.hip -- structural features of the loaded rows as a scalar set
// (include/bh_engine_posterior_features.h).
//
// One lane per loaded row, as sc_moho_kernel: the lane walks its row once per feature of the call's table and writes the
// feature's one or two columns, val[c * nrows + r] -- consecutive lanes to consecutive addresses, one store per column and row.
// The kinds of the table are the same for every lane (scalar loads); a (site, feature)'s three parameters are read by every
// lane at its own site's address: rows lie grouped by site, so all but the wavefronts that straddle a site boundary read one
// address, which the memory pipeline serves as one broadcast.  Row values are read inside the loops (an L1 / L2 hit after the
// first feature touched the row): no private array, no scratch.  The per-column counts of rows with a value meet in the
// wave-aggregated integer atomics of posterior_common.h; nothing else leaves a lane, so a site's columns are the same bits in
// every run, alone or among other sites.
// -ffp-contract=off (Makefile): no product or quotient of a layer is contracted into its sum.
#include "posterior_common.h"
#include "../../include/bh_engine_posterior_features.h"

#include <cmath>

using namespace bhpost;

namespace {

__device__ __forceinline__ double ft_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ double ft_inf() { return __longlong_as_double(0x7ff0000000000000ll); }
__device__ __forceinline__ double ft_finite(double v) { return fabs(v) < ft_inf() ? v : ft_nan(); }

template <typename T>
__global__ void __launch_bounds__(256) ft_features_kernel(int64_t nrows, int ML, const int32_t *__restrict__ pn,
                                                          const int32_t *__restrict__ psite, const T *__restrict__ pvs,
                                                          const double *__restrict__ pd, int F, int ncols,
                                                          const int32_t *__restrict__ kind, const int32_t *__restrict__ col0,
                                                          const double *__restrict__ par, double *__restrict__ val,
                                                          unsigned long long *found)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool act = r < nrows;
    const int64_t rr = act ? r : 0;
    const int s = act ? psite[rr] : 0;
    const int n = act ? pn[rr] : 0; // (a lane past the rows walks nothing and only takes part in the counts)
    const T *vs = pvs + rr * ML;
    const double *d = pd + rr * ML;
    for (int f = 0; f < F; ++f) {
        const int kd = kind[f], c0 = col0[f];
        const double *pp = par + ((size_t)s * F + f) * 3;
        const double z0 = pp[0], z1 = pp[1], c = pp[2];
        double a = ft_nan(), b = ft_nan();
        bool two = false;
        if (kd <= BH_FEATURE_TTS) {
            double sum = 0.0, t = 0.0;
            for (int j = 0; j < n; ++j) {
                const double bj = j < n - 1 ? d[j] : ft_inf();
                const double len = fmin(bj, z1) - fmax(t, z0);
                if (len > 0.0) {
                    const double v = (double)vs[j];
                    sum = sum + (kd == BH_FEATURE_VSMEAN ? v * len : len / v);
                }
                t = bj;
            }
            a = kd == BH_FEATURE_VSMEAN ? sum / (z1 - z0) : kd == BH_FEATURE_VSTIME ? (z1 - z0) / sum : sum;
        } else if (kd <= BH_FEATURE_VSMAX) {
            two = true;
            const bool mx = kd == BH_FEATURE_VSMAX;
            bool have = false;
            double t = 0.0;
            for (int j = 0; j < n; ++j) {
                const double bj = j < n - 1 ? d[j] : ft_inf();
                const double top = fmax(t, z0);
                const double len = fmin(bj, z1) - top;
                if (len > 0.0) {
                    const double v = (double)vs[j];
                    if (!have || (mx ? v > a : v < a)) {
                        a = v;
                        b = top;
                        have = true;
                    }
                }
                t = bj;
            }
        } else if (kd <= BH_FEATURE_JUMP) {
            two = true;
            const bool up = kd == BH_FEATURE_JUMP;
            bool have = false;
            double best = 0.0, dep = 0.0;
            for (int k = 0; k < n - 1; ++k) {
                const double dk = d[k];
                if (dk > z0 && dk < z1) {
                    const double jm = (double)(T)(vs[k + 1] - vs[k]);
                    if (!have || (up ? jm > best : jm < best)) {
                        best = jm;
                        dep = dk;
                        have = true;
                    }
                }
            }
            if (have && (up ? best > c : best < -c)) {
                a = dep;
                b = best;
            }
        } else if (kd == BH_FEATURE_ABOVE) {
            int k = -1;
            for (int j = n - 2; j >= 0; --j) k = (d[j] > z0 && d[j] < z1 && (double)vs[j + 1] > c) ? j : k;
            if (k >= 0) a = d[k];
        } else {
            int cnt = 0;
            for (int k = 0; k < n - 1; ++k) cnt += (d[k] > z0 && d[k] < z1) ? 1 : 0;
            a = (double)cnt;
        }
        a = ft_finite(a);
        b = ft_finite(b);
        if (act) {
            val[(int64_t)c0 * nrows + r] = a;
            if (two) val[(int64_t)(c0 + 1) * nrows + r] = b;
        }
        agg_add(found, s * ncols + c0, act && a == a);
        if (two) agg_add(found, s * ncols + c0 + 1, act && b == b); // (the kind is the wavefront's: every lane calls)
    }
}

inline int kind_cols(int k) { return (k >= BH_FEATURE_VSMIN && k <= BH_FEATURE_JUMP) ? 2 : 1; }

} // namespace

extern "C" int bh_posterior_features(bh_posterior *p, int F, const int32_t *kind, const double *par, int64_t *found)
{
    int rc;
    if (!p) return BH_EINVAL;
    if (p->S < 1) return pfail(p, BH_EINVAL, "no rows loaded (bh_posterior_load)");
    if (!p->has_rows) return pfail(p, BH_EINVAL, "the rows were loaded without bh_posterior_keep_rows");
    if (F < 1 || F > BH_FEATURES_MAXKINDS) return pfail(p, BH_EINVAL, "F: 1..64 features in one call");
    if (!kind || !par) return pfail(p, BH_EINVAL, "null argument");
    const int S = p->S;
    std::vector<int32_t> c0(F);
    int ncols = 0;
    for (int f = 0; f < F; ++f) {
        if (kind[f] < BH_FEATURE_VSMEAN || kind[f] > BH_FEATURE_NIFACES)
            return pfail(p, BH_EINVAL, "kind[" + std::to_string(f) + "]: no such feature kind");
        c0[f] = ncols;
        ncols += kind_cols(kind[f]);
    }
    if (ncols > BH_SCALARS_MAXCOLS) return pfail(p, BH_EINVAL, "kind: the features have more than BH_SCALARS_MAXCOLS (64) columns");
    if ((int64_t)S * ncols > (int64_t)INT_MAX) return pfail(p, BH_EINVAL, "nsites * columns must stay below 2^31");
    for (int s = 0; s < S; ++s)
        for (int f = 0; f < F; ++f) {
            const double *q = par + ((size_t)s * F + f) * 3;
            const std::string at = "par[" + std::to_string(s) + "][" + std::to_string(f) + "]";
            if (!std::isfinite(q[0]) || !std::isfinite(q[1]) || !std::isfinite(q[2]))
                return pfail(p, BH_EINVAL, at + ": z0, z1 and c must be finite");
            if (q[0] < 0.0) return pfail(p, BH_EINVAL, at + ": z0 must not lie below 0 km");
            if (!(q[1] > q[0])) return pfail(p, BH_EINVAL, at + ": the window needs z0 < z1");
            if ((kind[f] == BH_FEATURE_DROP || kind[f] == BH_FEATURE_JUMP) && q[2] < 0.0)
                return pfail(p, BH_EINVAL, at + ": c must not be negative for a drop or a jump");
        }
    PCHK(p, hipSetDevice(p->device));
    ScalarSet &ss = p->sets[set_slot(BH_SCALARS_FEATURES)];
    ss.drop();
    const size_t nr = (size_t)p->nrows, ncnt = (size_t)S * ncols, npar = (size_t)S * F * 3;
    Dev dkind, dc0, dpar, dfound;
    if ((rc = alloc(p, ss.val, nr * ncols * 8)) || (rc = alloc(p, dkind, (size_t)F * 4)) || (rc = alloc(p, dc0, (size_t)F * 4)) ||
        (rc = alloc(p, dpar, npar * 8)) || (rc = alloc(p, dfound, ncnt * 8)))
        return rc;
    PCHK(p, hipMemcpyAsync(dkind.p, kind, (size_t)F * 4, hipMemcpyHostToDevice, p->st));
    PCHK(p, hipMemcpyAsync(dc0.p, c0.data(), (size_t)F * 4, hipMemcpyHostToDevice, p->st));
    PCHK(p, hipMemcpyAsync(dpar.p, par, npar * 8, hipMemcpyHostToDevice, p->st));
    PCHK(p, hipMemsetAsync(dfound.p, 0, ncnt * 8, p->st));
    if (nr) {
        const unsigned nblk = (unsigned)((nr + 255) / 256);
        if (p->elem == 4)
            ft_features_kernel<float><<<nblk, 256, 0, p->st>>>(p->nrows, p->ML, p->pn.as<int32_t>(), p->psite.as<int32_t>(), p->pvs.as<float>(),
                p->pd.as<double>(), F, ncols, dkind.as<int32_t>(), dc0.as<int32_t>(), dpar.as<double>(), ss.val.as<double>(),
                dfound.as<unsigned long long>());
        else
            ft_features_kernel<double><<<nblk, 256, 0, p->st>>>(p->nrows, p->ML, p->pn.as<int32_t>(), p->psite.as<int32_t>(), p->pvs.as<double>(),
                p->pd.as<double>(), F, ncols, dkind.as<int32_t>(), dc0.as<int32_t>(), dpar.as<double>(), ss.val.as<double>(),
                dfound.as<unsigned long long>());
        PCHK(p, hipGetLastError());
    }
    std::vector<unsigned long long> hf(ncnt);
    PCHK(p, hipMemcpyAsync(hf.data(), dfound.p, ncnt * 8, hipMemcpyDeviceToHost, p->st));
    PCHK(p, hipStreamSynchronize(p->st));
    if (found)
        for (size_t i = 0; i < ncnt; ++i) found[i] = (int64_t)hf[i];
    ss.Q = ncols;
    return BH_OK;
}
