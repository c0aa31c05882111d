"""The refusals of the chain-diagnostics entry points, entry point by entry point, against tests/golden/chain_diag_refusals_golden.npz:
what the twelve entry points of the commit before csrc/chain_tables.h returned -- the code and the engine's last error --, row by row.

The table was recorded once on an MI355X from that commit's built library through its public entry points, by a throw-away script
that was never committed.  Per entry point the script took four calls in order (C = 1, 4, 6, 9 chains, both memory spaces, both
element sizes, padded and unpadded leading dimensions) and drew rows around one argument rule at a time -- several values of the
violating field on each of the four -- and rows that violate two rules at once, every ordered pair of the entry's rules on two of the
calls, so that the order of the checks is pinned.  A call was issued only after a restatement of the entry's checks had found that the
row violates a rule checked before hipSetDevice: no recorded call touched the device, and an engine is all that needs the GPU here.
The vectors the rules read on the host (ladder or group, dep, zoff) are real arrays of the table; every other pointer is null or the
address of a small host buffer that is never read.

Asserted: code and text of every row; that every entry point occurs with every refusal text its source has before the first HIP
call; and (tests/test_chain_tables.py, without a GPU) that the rows refused by a rule of csrc/chain_tables.h get the same answer from
the pure function."""
import pytest

from conftest import golden
from test_chain_tables import (ENTRIES, GROUP_TEXTS, MODEL_TEXTS, T_LSPAN, T_SEL, T_SPAN, call_entry, table_rows)

pytestmark = pytest.mark.gpu

ELEM, NULL, LAG, COLS = "the table must be float32 or float64", "null argument", "maxlag must be 0..BH_DIAG_MAXLAG", "columns: 1..BH_DIAG_MAXCOLS per call"
RANK = ("z and zf need the table zt and its offsets zoff", "T * C must stay below 2^32", "bad leading dimensions of the outputs",
        "groups: 1 <= G <= C", "a group value outside [-1, G)", "an empty group", "a zoff that does not fit (0 .. 2^40)")
# the refusal texts of every entry point's source before its first HIP call
TEXTS = {
    "bh_chain_diag_series": (ELEM, NULL, LAG, COLS, T_SPAN),
    "bh_chain_diag_models": (ELEM, NULL, LAG, T_SPAN) + MODEL_TEXTS,
    "bh_chain_diag_medians": (ELEM, NULL, T_SPAN),
    "bh_chain_diag_series_sel": (ELEM, NULL, LAG, COLS, T_SPAN, T_SEL),
    "bh_chain_diag_models_sel": (ELEM, NULL, LAG, T_SPAN, T_SEL) + MODEL_TEXTS,
    "bh_chain_diag_medians_sel": (ELEM, NULL, T_SPAN, T_SEL),
    "bh_chain_ladder_index": (NULL, T_LSPAN) + GROUP_TEXTS,
    "bh_chain_ladder_holders": (NULL, T_LSPAN) + GROUP_TEXTS,
    "bh_chain_ladder_evidence": (NULL, "the likes must be float32 or float64", T_LSPAN) + GROUP_TEXTS,
    "bh_chain_rank_series": (ELEM, NULL, COLS, T_SPAN) + RANK,
    "bh_chain_rank_models": (ELEM, NULL, "columns: q0 .. q0 + nq - 1 within 0 .. D", T_SPAN) + MODEL_TEXTS + RANK,
    "bh_ladder_sweep_create": (NULL, "bad C or K") + GROUP_TEXTS[:3],
}


def test_refusals_equal_the_parent_commits_row_by_row():
    from bayhunter_amd import engine as E
    eng = E.Engine(0)
    seen = {e: set() for e in ENTRIES}
    rows = 0
    for i, row in table_rows(golden("chain_diag_refusals_golden.npz")):
        name = ENTRIES[row["entry"]]
        assert row["code"] != E.BH_OK
        got = call_entry(eng._L, eng._h, row)
        assert got == (row["code"], row["text"]), "row %d of %s: %r, recorded %r" % (i, name, got, (row["code"], row["text"]))
        seen[name].add(row["text"])
        rows += 1
    assert rows > 12 * 100
    for e in ENTRIES:
        assert seen[e] == set(TEXTS[e]), (e, seen[e] ^ set(TEXTS[e]))
