// bayhunter_amd/csrc/chain_tables.hip -- the argument rules of the chain-diagnostics entry points (chain_tables.h), each once.
// Host code only: no kernel, no HIP call, nothing static -- every answer is a function of the arguments alone.
#include "chain_tables.h"
#include "../../include/bh_engine_chain_diag_ladders.h"

#include <cmath>

namespace {

const bh_chain_refusal OK = {BH_OK, nullptr};

bh_chain_refusal refuse(int code, const char *text) { return bh_chain_refusal{code, text}; }

} // namespace

extern "C" {

bh_chain_refusal bh_chain_table_span(int64_t T, int C, int64_t width, int64_t ld_t, int64_t ld_c)
{
    const char *text = "bad T, C or leading dimensions";
    if (T < 1 || C < 1 || ld_t < 1 || ld_c < width) return refuse(BH_EINVAL, text);
    // the span in elements stays below 2^60
    const long double span = (long double)(T - 1) * (long double)ld_t + (long double)(C - 1) * (long double)ld_c + (long double)width;
    return span < 1.152921504606846976e18L ? OK : refuse(BH_EINVAL, text);
}

bh_chain_refusal bh_chain_sel_span(int64_t T, int K, int sel_not_null, int64_t ld_sel)
{
    if (K >= 1 && sel_not_null && ld_sel >= K && (long double)(T - 1) * (long double)ld_sel + (long double)K < 1.152921504606846976e18L)
        return OK;
    return refuse(BH_EINVAL, "the selection: K >= 1 series, ld_sel >= K");
}

bh_chain_refusal bh_chain_ladder_span(int64_t T, int64_t ld_t, int C, int64_t ld_c)
{
    // the span in elements stays below 2^40
    if ((long double)T * (long double)ld_t + (long double)C * (long double)ld_c >= 1099511627776.0L)
        return refuse(BH_EINVAL, "bad T, C, K or leading dimensions");
    return OK;
}

bh_chain_refusal bh_chain_model_table(int ML, int D, const double *dep)
{
    if (ML < 1 || ML > BH_POSTERIOR_MAXLAYERS) return refuse(BH_EINVAL, "row width 2*ML must be 2..64 (ML <= BH_POSTERIOR_MAXLAYERS)");
    if (D < 0 || D > BH_DIAG_MAXDEPTHS || (D && !dep)) return refuse(BH_EINVAL, "depths: 0..BH_DIAG_MAXDEPTHS");
    for (int j = 0; j < D; ++j)
        if (!std::isfinite(dep[j]) || (j && !(dep[j] > dep[j - 1])))
            return refuse(BH_EINVAL, "the depths must be finite and strictly ascending");
    return OK;
}

bh_chain_refusal bh_chain_ladder_groups(int C, const int32_t *ladder, int K, const int *R, int32_t *start, int32_t *member, int *largest)
{
    for (int k = 0; k <= K; ++k) start[k] = 0;
    for (int c = 0; c < C; ++c) {
        if (ladder[c] < 0 || ladder[c] >= K) return refuse(BH_EINVAL, "ladder ids must be 0..K-1");
        ++start[ladder[c] + 1];
    }
    int most = 0;
    for (int k = 0; k < K; ++k) {
        if (!start[k + 1]) return refuse(BH_EINVAL, "ladder ids must be 0..K-1, every id used");
        most = start[k + 1] > most ? start[k + 1] : most;
    }
    if (most > BH_LADDER_MAXRUNGS) return refuse(BH_EUNSUPPORTED, "a ladder of more than BH_LADDER_MAXRUNGS chains");
    if (R && *R != most) return refuse(BH_EINVAL, "R must be the size of the largest ladder");
    if (largest) *largest = most;
    // the counts become the ladders' first places; a ladder's members follow in ascending chain order
    for (int k = 0; k < K; ++k) start[k + 1] += start[k];
    // (start[k] walks through ladder k's places, ends at the next ladder's first and is moved back)
    for (int c = 0; c < C; ++c) member[start[ladder[c]]++] = c;
    for (int k = K; k > 0; --k) start[k] = start[k - 1];
    start[0] = 0;
    return OK;
}

} // extern "C"
