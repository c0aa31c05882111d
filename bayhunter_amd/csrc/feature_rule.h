// bayhunter_amd/csrc/feature_rule.h -- the rule of the structural features (include/bh_engine_posterior_features.h), stated once: the
// device code that posterior_features_kernel.hip (the rows a bh_posterior handle has loaded) and chain_diag_features_kernel.hip (the
// rows of the chains' store, where they lie) share, so that both give the same bits; and the host check of the table of kinds and
// parameters that both entry points make, with its messages.
//
// The walk is parametrised over how a row gives its numbers.  A row type R has
//     T vs(int j) const          vs_j in the row's dtype
//     R::Depths                  a cursor built from the row whose next() returns d_0, d_1, .. in turn (float64)
// and every kind reads the interfaces in ascending order, once: a loaded row reads the d the load stored (LoadedRow), a store row
// forms them on the way from its z (StoreRow: zd_j = (z_j + z_{j+1}) / 2 in the row's type, d_j the float64 running sum -- the rule of
// bh_engine_posterior.h, post_scatter_kernel's statements).  No private array, nothing indexed dynamically: no scratch.
// -ffp-contract=off (Makefile): no product or quotient of a layer is contracted into its sum.
#ifndef BH_FEATURE_RULE_H
#define BH_FEATURE_RULE_H

#include "../../include/bh_engine_posterior_features.h"

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

__device__ __forceinline__ double ft_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ double ft_inf() { return __longlong_as_double(0x7ff0000000000000ll); }
__device__ __forceinline__ double ft_finite(double v) { return fabs(v) < ft_inf() ? v : ft_nan(); }

// a row of a loaded handle: vs [n] in the row's dtype and d [n-1] as bh_posterior_load stored them
template <typename T> struct LoadedRow {
    const T *v;
    const double *d;
    __device__ __forceinline__ T vs(int j) const { return v[j]; }
    struct Depths {
        const double *p;
        __device__ __forceinline__ explicit Depths(const LoadedRow &r) : p(r.d) {}
        __device__ __forceinline__ double next() { return *p++; }
    };
};

// a row of the store, [vs_1..vs_n, z_1..z_n, NaN..]: the depths are formed as they are asked for
template <typename T> struct StoreRow {
    const T *row;
    int n;
    __device__ __forceinline__ T vs(int j) const { return row[j]; }
    struct Depths {
        const T *z;
        T zprev;
        double dsum;
        int j;
        __device__ __forceinline__ explicit Depths(const StoreRow &r) : z(r.row + r.n), zprev((T)0), dsum(0.0), j(0) {}
        __device__ __forceinline__ double next()
        {
            const T zd = (z[j] + z[j + 1]) / (T)2;
            const double h = (double)zd - (double)zprev;
            dsum = j ? dsum + h : h;
            zprev = zd;
            ++j;
            return dsum;
        }
    };
};

// The one or two columns (a, b) of a feature of kind kd with the parameters (z0, z1, c) for a row of n layers; NaN where the row lacks
// the column or the result is not finite.  Returns whether the kind has two columns.
template <typename T, typename R>
__device__ __forceinline__ bool feature_columns(int kd, int n, const R &row, double z0, double z1, double c, double &a, double &b)
{
    typename R::Depths dc(row);
    bool two = false;
    a = ft_nan();
    b = ft_nan();
    if (kd <= BH_FEATURE_TTS) {
        double sum = 0.0, t = 0.0;
        for (int j = 0; j < n; ++j) {
            const double bj = j < n - 1 ? dc.next() : ft_inf();
            const double len = fmin(bj, z1) - fmax(t, z0);
            if (len > 0.0) {
                const double v = (double)row.vs(j);
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
            const double bj = j < n - 1 ? dc.next() : ft_inf();
            const double top = fmax(t, z0);
            const double len = fmin(bj, z1) - top;
            if (len > 0.0) {
                const double v = (double)row.vs(j);
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
            const double dk = dc.next();
            if (dk > z0 && dk < z1) {
                const double jm = (double)(T)(row.vs(k + 1) - row.vs(k));
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
        bool have = false;   // the smallest k in the window with vs_{k+1} > c
        for (int k = 0; k < n - 1; ++k) {
            const double dk = dc.next();
            if (!have && dk > z0 && dk < z1 && (double)row.vs(k + 1) > c) {
                a = dk;
                have = true;
            }
        }
    } else {
        int cnt = 0;
        for (int k = 0; k < n - 1; ++k) {
            const double dk = dc.next();
            cnt += (dk > z0 && dk < z1) ? 1 : 0;
        }
        a = (double)cnt;
    }
    a = ft_finite(a);
    b = ft_finite(b);
    return two;
}

inline int feature_kind_cols(int k) { return (k >= BH_FEATURE_VSMIN && k <= BH_FEATURE_JUMP) ? 2 : 1; }

// The table of kinds and parameters of a call over S sites: BH_OK with col0 [F] and the number of columns, or BH_EINVAL with the
// refusal's text -- the checks of bh_posterior_features, in their order.
inline int feature_table(int F, const int32_t *kind, const double *par, int S, std::vector<int32_t> &col0, int &ncols, std::string &what)
{
    if (F < 1 || F > BH_FEATURES_MAXKINDS) { what = "F: 1..64 features in one call"; return BH_EINVAL; }
    if (!kind || !par) { what = "null argument"; return BH_EINVAL; }
    col0.assign((size_t)F, 0);
    ncols = 0;
    for (int f = 0; f < F; ++f) {
        if (kind[f] < BH_FEATURE_VSMEAN || kind[f] > BH_FEATURE_NIFACES) {
            what = "kind[" + std::to_string(f) + "]: no such feature kind";
            return BH_EINVAL;
        }
        col0[(size_t)f] = ncols;
        ncols += feature_kind_cols(kind[f]);
    }
    if (ncols > BH_SCALARS_MAXCOLS) { what = "kind: the features have more than BH_SCALARS_MAXCOLS (64) columns"; return BH_EINVAL; }
    if ((int64_t)S * ncols > (int64_t)INT_MAX) { what = "nsites * columns must stay below 2^31"; return BH_EINVAL; }
    for (int s = 0; s < S; ++s)
        for (int f = 0; f < F; ++f) {
            const double *q = par + ((size_t)s * F + f) * 3;
            const std::string at = "par[" + std::to_string(s) + "][" + std::to_string(f) + "]";
            if (!std::isfinite(q[0]) || !std::isfinite(q[1]) || !std::isfinite(q[2])) { what = at + ": z0, z1 and c must be finite"; return BH_EINVAL; }
            if (q[0] < 0.0) { what = at + ": z0 must not lie below 0 km"; return BH_EINVAL; }
            if (!(q[1] > q[0])) { what = at + ": the window needs z0 < z1"; return BH_EINVAL; }
            if ((kind[f] == BH_FEATURE_DROP || kind[f] == BH_FEATURE_JUMP) && q[2] < 0.0) {
                what = at + ": c must not be negative for a drop or a jump";
                return BH_EINVAL;
            }
        }
    return BH_OK;
}

#endif
