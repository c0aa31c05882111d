// bayhunter_amd/csrc/posterior_features_kernel.hip -- structural features of the loaded rows as a scalar set
// (include/bh_engine_posterior_features.h).
//
// One lane per loaded row, as sc_moho_kernel: the lane walks its row once per feature of the call's table and writes the
// feature's one or two columns, val[c * nrows + r] -- consecutive lanes to consecutive addresses, one store per column and row.
// The kinds of the table are the same for every lane (scalar loads); a (site, feature)'s three parameters are read by every
// lane at its own site's address: rows lie grouped by site, so all but the wavefronts that straddle a site boundary read one
// address, which the memory pipeline serves as one broadcast.  The walk of a row is feature_rule.h's, shared with the series of the
// chains' store (chain_diag_features_kernel.hip): row values are read inside the loops (an L1 / L2 hit after the first feature
// touched the row): no private array, no scratch.  The per-column counts of rows with a value meet in the
// wave-aggregated integer atomics of posterior_common.h; nothing else leaves a lane, so a site's columns are the same bits in
// every run, alone or among other sites.
// -ffp-contract=off (Makefile): no product or quotient of a layer is contracted into its sum.
#include "posterior_common.h"
#include "feature_rule.h"
#include "../../include/bh_engine_posterior_features.h"

#include <cmath>

using namespace bhpost;

namespace {

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
    const LoadedRow<T> row = {pvs + rr * ML, pd + rr * ML};
    for (int f = 0; f < F; ++f) {
        const int kd = kind[f], c0 = col0[f];
        const double *pp = par + ((size_t)s * F + f) * 3;
        double a, b;
        const bool two = feature_columns<T>(kd, n, row, pp[0], pp[1], pp[2], a, b);   // (feature_rule.h: the rule, stated once)
        if (act) {
            val[(int64_t)c0 * nrows + r] = a;
            if (two) val[(int64_t)(c0 + 1) * nrows + r] = b;
        }
        agg_add(found, s * ncols + c0, act && a == a);
        if (two) agg_add(found, s * ncols + c0 + 1, act && b == b); // (the kind is the wavefront's: every lane calls)
    }
}

} // namespace

extern "C" int bh_posterior_features(bh_posterior *p, int F, const int32_t *kind, const double *par, int64_t *found)
{
    int rc;
    if (!p) return BH_EINVAL;
    if (p->S < 1) return pfail(p, BH_EINVAL, "no rows loaded (bh_posterior_load)");
    if (!p->has_rows) return pfail(p, BH_EINVAL, "the rows were loaded without bh_posterior_keep_rows");
    const int S = p->S;
    std::vector<int32_t> c0;
    std::string what;
    int ncols = 0;
    if ((rc = feature_table(F, kind, par, S, c0, ncols, what))) return pfail(p, rc, what);
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
