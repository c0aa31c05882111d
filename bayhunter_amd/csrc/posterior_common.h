// bayhunter_amd/csrc/posterior_common.h -- what posterior_kernel.hip, posterior_scalars_kernel.hip, posterior_datafit_kernel.hip,
// posterior_features_kernel.hip, posterior_classes_kernel.hip and posterior_resid_kernel.hip share: the handle, its device buffers, the work items, the ordered keys and the bin rule.
#ifndef BH_POSTERIOR_COMMON_H
#define BH_POSTERIOR_COMMON_H

#include "bh_hostkit.h"
#include "bh_okey.h"
#include "../../include/bh_engine_posterior.h"

#include <climits>
#include <string>
#include <vector>

#define POST_CHUNK 8192  // rows per workgroup of a column pass (< 2^16: the radix pass's 16-bit LDS counters)

namespace bhpost {

struct PostWork {
    int32_t site, pad;
    int64_t r0, r1;
};

__device__ __forceinline__ unsigned long long lanes_below() { return (1ull << __lane_id()) - 1ull; }

// ctr[key] += 1 for every lane with `on`, one atomic per distinct key of the wavefront; returns the lane's old value +
// its rank among the lanes of its key.  Every lane of the wavefront must call it.
__device__ inline unsigned long long agg_add(unsigned long long *ctr, int key, bool on)
{
    unsigned long long res = 0, pending = __ballot(on);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const int lkey = __shfl(key, leader);
        const bool mine = on && key == lkey && ((pending >> __lane_id()) & 1ull);
        const unsigned long long m = __ballot(mine);
        unsigned long long base = 0;
        if (__lane_id() == leader) base = atomicAdd(&ctr[lkey], (unsigned long long)__popcll(m));
        base = __shfl(base, leader);
        if (mine) res = base + (unsigned long long)__popcll(m & lanes_below());
        pending &= ~m;
    }
    return res;
}

// the ordered key of v (bh_okey.h): of its float32 value where the column's values are float32-exact, else of the double
__device__ __forceinline__ unsigned long long okey(double v, bool k32) { return k32 ? (unsigned long long)okey32((float)v) : okey64(v); }

// exponent of the lowest set bit of v (INT_MAX for 0)
__device__ __forceinline__ int low_bit(double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const int ex = (int)((u >> 52) & 0x7ff);
    unsigned long long m = u & 0xfffffffffffffull;
    if (ex) m |= 1ull << 52;
    if (!m) return INT_MAX;
    return (ex ? ex - 1075 : -1074) + __ffsll((long long)m) - 1;
}

// bin of v over e[0..nb]: searchsorted(e, v, 'right') - 1, the last edge into the last bin; -1 / nb outside
__device__ __forceinline__ int find_bin(const double *e, int nb, double v)
{
    int lo = 0, hi = nb + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= v) lo = mid + 1;
        else hi = mid;
    }
    return (v == e[nb]) ? nb - 1 : lo - 1;
}

typedef bhkit::Buf Dev;

// a scalar set (include/bh_engine_posterior_scalars.h): Q float64 columns over the loaded rows, val[q * nrows + r], NaN = masked
struct ScalarSet {
    int Q = 0;
    Dev val;
    // what the last bh_posterior_scalar_stats of the set found (empty: none since the set was formed): every (site, column)'s
    // count and every column's "not float32-exact" flag -- bh_posterior_scalar_quantiles checks its ranks and sizes its keys by them
    std::vector<int64_t> count;
    std::vector<int32_t> nf;
    void drop()
    {
        Q = 0;
        count.clear();
        nf.clear();
    }
};

// the handle's slot of a set id (include/bh_engine_posterior_datafit.h: MOHO 0, USER 1, DATA 3; include/bh_engine_posterior_features.h:
// FEATURES 4; include/bh_engine_posterior_resid.h: RESID 5); -1: no such set
inline int set_slot(int set) { return set == 0 ? 0 : set == 1 ? 1 : set == 3 ? 2 : set == 4 ? 3 : set == 5 ? 4 : -1; }

} // namespace bhpost

struct bh_posterior {
    bh_engine *e = nullptr;
    int device = 0;
    hipStream_t st = nullptr;
    int elem = 8, ML = 0, S = 0;
    int64_t nrows = 0, ninput = 0;
    bool keys32 = false;
    std::vector<int64_t> off;             // [S+1]: site s holds rows [off[s], off[s+1])
    std::vector<bhpost::PostWork> work;   // column-pass work items (site, chunk of its rows)
    bhpost::Dev pn, psite, pvs, pd, pdi, dwork;
    bool keep_rows = false;               // bh_posterior_keep_rows: the next load keeps porig and pzd
    bool has_rows = false;                // ... and the last one did
    bhpost::Dev porig, pzd;               // the row's index in the loaded input; zd_j in the row's dtype (the scalar sets)
    bhpost::ScalarSet sets[5];            // BH_SCALARS_MOHO, BH_SCALARS_USER, BH_SCALARS_DATA, BH_SCALARS_FEATURES, BH_SCALARS_RESID (bhpost::set_slot)
    int data_ldy = 0;                     // bh_posterior_data_fill: the columns of the set being filled, the rows filled so far,
    int64_t data_filled = -1;             // (-1: no fill under way) and the failed rows per site
    bhpost::Dev data_failed;
    bhpost::Dev data_tab;                 // ... and its tables (ncol, the columns' target and index in it), uploaded by the call that starts it
    std::vector<int32_t> data_ncol;       // (the host copy: the following calls must bring the same table)
    int resid_ldy = 0, resid_nt = 0, resid_L = 0;   // bh_posterior_resid_fill (include/bh_engine_posterior_resid.h): what the call that
    int64_t resid_filled = -1;            // started the fill brought, the rows filled so far (-1: no fill under way), the failed rows
    bhpost::Dev resid_failed;             // per site,
    bhpost::Dev resid_tab;                // its int32 tables (ncol, every slot's first column), its float64 tables (yobs, then g
    bhpost::Dev resid_obs;                // where given) and a host noise table's copy;
    bhpost::Dev resid_noise;
    std::vector<int32_t> resid_ncol;      // the host copies the following calls' tables are compared with, and the kind of the
    std::vector<double> resid_host;       // noise table (memspace, element bytes, leading dimension)
    bool resid_g = false;
    int resid_nmem = 0, resid_nelem = 0;
    int64_t resid_nld = 0;
    bhpost::Dev mantle_tab;               // bh_posterior_layers: the last mantle table on the device, and the host copy it is compared with
    std::vector<double> mantle_host;
};

namespace bhpost {

// the kit (bh_hostkit.h) through the handle's engine
inline int pfail(bh_posterior *p, int code, const std::string &what) { return bhkit::fail(p->e, code, what); }

#define PCHK(p, call) BH_CHK((p)->e, call)

// (a buffer of the handle is allocated anew: what it held goes first)
inline int alloc(bh_posterior *p, Dev &b, size_t bytes)
{
    if (b.p) { (void)hipFree(b.p); b.p = nullptr; }
    return bhkit::alloc(p->e, b, bytes);
}

} // namespace bhpost
#endif
