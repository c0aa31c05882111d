// bayhunter_amd/csrc/chain_diag_value.h -- the value a model row contributes to the chains' series: the device code that
// chain_diag_kernel.hip (the sums) and chain_rank_kernel.hip (the rank transform) share, so that both see the same numbers.
#ifndef BH_CHAIN_DIAG_VALUE_H
#define BH_CHAIN_DIAG_VALUE_H

// Column q of a model row [vs_1..vs_n, z_1..z_n, NaN...] of 2*ML values: q < D the vs at depth dep[q] -- vs[#{j : d_j <= dep[q]}]
// (the rule of bh_engine_posterior.h, posterior_kernel.hip) --, q == D: n - 1.  CHECK: a non-NaN value beyond `big` sets bad |= 1;
// a row whose non-NaN values are not a non-empty prefix of even length sets bad |= 2 (always) and gives 0.
template <typename T, bool CHECK>
__device__ __forceinline__ double diag_model_value(const T *row, int ML, int D, const double *dep, int q, double big, int &bad)
{
    const int W = 2 * ML;
    int cnt = 0, first = W;
    for (int i = 0; i < W; ++i) {
        const T v = row[i];
        const bool nan = v != v;
        cnt += nan ? 0 : 1;
        first = (nan && i < first) ? i : first;
        if (CHECK && !nan && !(fabs((double)v) <= big)) bad |= 1;
    }
    if (cnt == 0 || cnt != first || (cnt & 1)) {
        bad |= 2;
        return 0.0;
    }
    const int n = cnt / 2;
    if (q == D) return (double)(n - 1);
    const double xq = dep[q];
    const T *z = row + n;
    T zprev = (T)0;
    double dsum = 0.0;
    int k = 0;
    for (int j = 0; j < n - 1; ++j) {
        const T zd = (z[j] + z[j + 1]) / (T)2;
        const double h = (double)zd - (double)zprev;
        dsum = j ? dsum + h : h;
        k += dsum <= xq ? 1 : 0;
        zprev = zd;
    }
    return (double)row[k];
}

#endif
