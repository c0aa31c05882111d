// bayhunter_amd/csrc/chain_tables.h -- the argument rules of the chain-diagnostics entry points (include/bh_engine_chain_diag.h,
// bh_engine_chain_diag_ladders.h, bh_engine_chain_rank.h, bh_engine_chain_ladder_sweep.h, bh_engine_chain_ladder_evidence.h), each
// stated once.
//
// Host only, no HIP type, no engine (chain_tables.hip; pure: no HIP call, nothing static): a rule answers with a code and the text
// of the refusal, and the entry point that asks keeps the order of its checks and any text of its own.  The rules are exported
// (C linkage), so tests/test_chain_tables.py holds them to a restatement without a GPU.
#ifndef BH_CHAIN_TABLES_H
#define BH_CHAIN_TABLES_H

#include "../../include/bh_engine.h"

struct bh_chain_refusal {
    int code;           // BH_OK, or the code of the refusal
    const char *text;   // the refusal's text (a literal); null with BH_OK
};

extern "C" {

// A table [T][C][width] of elements with the rows ld_t and the chains ld_c apart: T, C, ld_t >= 1, ld_c >= width, and the span
// (T-1) ld_t + (C-1) ld_c + width below 2^60 elements.  "bad T, C or leading dimensions".
bh_chain_refusal bh_chain_table_span(int64_t T, int C, int64_t width, int64_t ld_t, int64_t ld_c);

// A selection [T][K] with the rows ld_sel apart: K >= 1, a pointer, ld_sel >= K, (T-1) ld_sel + K below 2^60 (T >= 1: the table's
// rule comes first).  "the selection: K >= 1 series, ld_sel >= K".
bh_chain_refusal bh_chain_sel_span(int64_t T, int K, int sel_not_null, int64_t ld_sel);

// The ladder units' form, for tables they index with 40-bit products: T ld_t + C ld_c below 2^40 elements (a table of whole rows:
// C = 0, ld_c = 0).  "bad T, C, K or leading dimensions".
bh_chain_refusal bh_chain_ladder_span(int64_t T, int64_t ld_t, int C, int64_t ld_c);

// A table of model rows and the depths its columns are taken at: ML 1..BH_POSTERIOR_MAXLAYERS; D 0..BH_DIAG_MAXDEPTHS with dep
// where D > 0; dep finite and strictly ascending -- three refusals, in this order.
bh_chain_refusal bh_chain_model_table(int ML, int D, const double *dep);

// The ladders of C >= 1 chains, ladder[c] in 0..K-1 (K >= 1): start[K + 1] and member[C] -- the chains of ladder k are
// member[start[k] .. start[k+1]), ascending -- and, where asked for (not null), the size of the largest ladder.  Refused, in this
// order: an id outside 0..K-1, an id without a chain, a ladder of more than BH_LADDER_MAXRUNGS chains (BH_EUNSUPPORTED), and, where
// R is given (not null), an *R that is not the size of the largest ladder.  start and member hold nothing of use after a refusal.
bh_chain_refusal bh_chain_ladder_groups(int C, const int32_t *ladder, int K, const int *R, int32_t *start, int32_t *member, int *largest);

} // extern "C"
#endif
