"""tests/classes_ref.py, the restatement of include/bh_engine_posterior_classes.h that the GPU tests use as their oracle, on
hand-made rows whose classes can be read off; the header's constants against bayhunter_amd/engine.py; and every refusal of
check_classes, which is pure host code."""
import re

import numpy as np
import pytest

import classes_ref as CR
from conftest import REPO
from bayhunter_amd import engine as E
from bayhunter_amd.posterior import CLASS_OPS, check_classes

NAN, INF = np.nan, np.inf
LABELS = {"moho": (E.SCALARS_MOHO, 0), "vscrust": (E.SCALARS_MOHO, 2), "lvz.depth": (E.SCALARS_FEATURES, 0),
          "lvz.jump": (E.SCALARS_FEATURES, 1), "vpvs": (E.SCALARS_USER, 0), "nlayers": (E.SCALARS_USER, 1)}


def test_the_constants_mirror_the_header():
    txt = open(REPO + "/include/bh_engine_posterior_classes.h").read()
    defs = {k: int(v) for k, v in re.findall(r"^#define\s+(BH_[A-Z0-9_]+)\s+(-?\d+)\b", txt, flags=re.M)}
    assert defs == dict(BH_CLASSES_MAX=16, BH_CLASS_MAXTERMS=64, BH_CLASS_IN=0, BH_CLASS_HAS=1, BH_CLASS_LACKS=2)
    assert (E.CLASSES_MAX, E.CLASS_MAXTERMS, E.CLASS_IN, E.CLASS_HAS, E.CLASS_LACKS) == (16, 64, 0, 1, 2)
    assert CLASS_OPS == CR.OPS == ("in", "has", "lacks")
    body = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert sorted(set(re.findall(r"\b(bh_[a-z_0-9]+)\s*\(", body))) == sorted(E.POSTERIOR_CLASSES_SYMBOLS)


def test_hand_made_rows():
    #          row:   0     1     2     3     4     5     6     7
    moho = np.array([30.0, 36.0, 35.9, NAN, 45.0, 29.9, 33.0, 33.0])
    lvz = np.array([NAN, 12.0, NAN, 12.0, NAN, NAN, 8.0, 8.0])
    site = np.array([0, 0, 0, 0, 0, 0, 1, 1])
    loaded = np.array([1, 1, 1, 1, 1, 1, 1, 0], bool)
    terms = [(0, "moho", "in", 30.0, 36.0), (0, "lvz", "lacks", 0, 0),       # shallow Moho, no LVZ
             (1, "moho", "in", np.array([36.0, 30.0]), 45.0),                # deep Moho (site 1: from 30 km)
             (2, "moho", "lacks", 0, 0), (2, "lvz", "has", 0, 0)]            # no Moho but an LVZ
    cls, counts = CR.classify(dict(moho=moho, lvz=lvz), terms, 3, site, loaded, 2)
    # row 0: on lo, in.  row 1: on hi of class 0 -> out; on lo of class 1 -> in.  row 2: class 0.  row 3: class 2.  row 4: on hi of
    # class 1 -> none.  row 5: below.  row 6: site 1, has an LVZ -> not 0, its class 1 starts at 30.  row 7: not loaded.
    assert cls.tolist() == [0, 1, 0, 2, -1, -1, 1, -1] and cls.dtype == np.int32
    assert counts.tolist() == [[2, 1, 1, 2], [0, 1, 0, 0]]
    assert counts.sum(1).tolist() == [6, 1]


def test_a_class_without_terms_takes_what_is_left_and_the_first_match_wins():
    v = np.array([1.0, 2.0, NAN, 3.0])
    ones = np.ones(4, bool)
    cls, counts = CR.classify(dict(v=v), [(0, "v", "in", 2.0, INF), (2, "v", "has", 0, 0)], 3, None, ones, 1)
    assert cls.tolist() == [1, 0, 1, 0] and counts.tolist() == [[2, 2, 0, 0]]            # class 1 has no term: class 2 never reached
    cls, counts = CR.classify(dict(v=v), [], 1, None, ones, 1)
    assert cls.tolist() == [0, 0, 0, 0] and counts.tolist() == [[4, 0]]
    cls, _ = CR.classify(dict(v=v), [(0, "v", "in", -INF, INF), (1, "v", "lacks", 0, 0)], 2, None, ones, 1)
    assert cls.tolist() == [0, 0, 1, 0]                                                  # (-inf, inf) is "has"
    cls, _ = CR.classify(dict(v=v), [(0, "v", "in", 2.0, 2.0)], 1, None, ones, 1)
    assert cls.tolist() == [-1, -1, -1, -1]                                              # lo == hi: empty


def test_signed_zero_and_infinite_bounds():
    v = np.array([0.0, -0.0, 5e-324, -5e-324])
    ones = np.ones(4, bool)
    cls, _ = CR.classify(dict(v=v), [(0, "v", "in", -0.0, INF)], 1, None, ones, 1)
    assert cls.tolist() == [0, 0, 0, -1]                                                 # -0.0 <= 0.0
    cls, _ = CR.classify(dict(v=v), [(0, "v", "in", -INF, 0.0)], 1, None, ones, 1)
    assert cls.tolist() == [-1, -1, -1, 0]                                               # 0.0 < 0.0 is false, and so is -0.0 < 0.0
    assert CR.term_holds(NAN, "in", -INF, INF) is False and CR.term_holds(NAN, "lacks", 0, 0) is True


def test_rule_terms_reads_the_users_dict():
    names, terms = CR.rule_terms({"a": [("moho", 30, 36), ("lvz", "lacks")], "b": [], "c": [("lvz", "has")]})
    assert names == ["a", "b", "c"]
    assert terms == [(0, "moho", "in", 30, 36), (0, "lvz", "lacks", -INF, INF), (2, "lvz", "has", -INF, INF)]
    with pytest.raises(ValueError):
        CR.classify({}, [(1, "v", "has", 0, 0), (0, "v", "has", 0, 0)], 2, None, np.ones(1, bool), 1)


def test_check_classes_gives_the_arrays_of_the_c_call():
    names, tc, ts, tq, to, lo, hi = check_classes(
        {"shallow": [("moho", 30, [36, 38, 40]), ("lvz.depth", "lacks")], "rest": [], "deep": [("moho", [36, 38, 40], INF), ("nlayers", 3, 9)]},
        3, LABELS)
    assert names == ["shallow", "rest", "deep"]
    for a in (tc, ts, tq, to):
        assert a.dtype == np.int32
    assert tc.tolist() == [0, 0, 2, 2] and ts.tolist() == [0, 4, 0, 1] and tq.tolist() == [0, 0, 0, 1]
    assert to.tolist() == [E.CLASS_IN, E.CLASS_LACKS, E.CLASS_IN, E.CLASS_IN]
    assert lo.shape == hi.shape == (3, 4) and lo.dtype == hi.dtype == np.float64 and lo.flags.c_contiguous and hi.flags.c_contiguous
    assert lo[:, 0].tolist() == [30, 30, 30] and hi[:, 0].tolist() == [36, 38, 40]
    assert lo[:, 2].tolist() == [36, 38, 40] and np.isinf(hi[:, 2]).all()
    assert np.isneginf(lo[:, 1]).all() and np.isposinf(hi[:, 1]).all()                   # (not read for has / lacks)
    names, tc, ts, tq, to, lo, hi = check_classes({"all": []}, 2, LABELS)
    assert names == ["all"] and tc.size == 0 and lo.shape == (2, 0)
    # lo == hi is an empty class, not an error; infinities are bounds
    check_classes({"a": [("moho", 30, 30), ("moho", -INF, INF)]}, 1, LABELS)
    # 16 classes with 64 terms are the most a call takes
    check_classes({"c%d" % k: [("moho", k, k + 1)] * 4 for k in range(16)}, 1, LABELS)


@pytest.mark.parametrize("classes, S, text", [
    (None, 1, "dict name -> list of terms"),
    ({}, 1, "at least one entry"),
    ([("a", [])], 1, "dict name -> list of terms"),
    ({"c%d" % k: [] for k in range(17)}, 1, "class 'c16' is the first too many.*16"),
    ({"": []}, 1, "non-empty string"),
    ({3: []}, 1, "class 3: the name"),
    ({"a": "moho"}, 1, "class 'a': expected a list of terms"),
    ({"a": {"moho": 1}}, 1, "class 'a': expected a list of terms"),
    ({"a": 5}, 1, "class 'a': expected a list of terms"),
    ({"a": ["moho"]}, 1, "class 'a': a term is"),
    ({"a": [("moho",)]}, 1, "class 'a': a term is"),
    ({"a": [("moho", 1, 2, 3)]}, 1, "class 'a': a term is"),
    ({"a": [("mohoo", 1, 2)]}, 1, "class 'a': 'mohoo' is no column of this call.*moho, vscrust"),
    ({"a": [(0, 1, 2)]}, 1, "class 'a': 0 is no column"),
    ({"a": [("moho", "have")]}, 1, "class 'a', column 'moho'.*'has'.*'lacks'"),
    ({"a": [("moho", 1)]}, 1, "class 'a', column 'moho'.*'has'.*'lacks'"),
    ({"a": [("moho", "x", 2)]}, 1, "class 'a', column 'moho': lo must be a number"),
    ({"a": [("moho", 1, None)]}, 1, "class 'a', column 'moho'"),
    ({"a": [("moho", [1, 2], 3)]}, 3, r"class 'a', column 'moho': lo must be one number or one per site \(3 sites\)"),
    ({"a": [("moho", 1, np.ones((2, 2)))]}, 2, "class 'a', column 'moho': hi must be one number or one per site"),
    ({"ok": [], "b": [("moho", [1, NAN], 3)]}, 2, "class 'b', column 'moho', site 1: a bound is NaN"),
    ({"b": [("moho", 1, NAN)]}, 2, "class 'b', column 'moho', site 0: a bound is NaN"),
    ({"b": [("vscrust", [1, 2, 4], [2, 3, 3.5])]}, 3, "class 'b', column 'vscrust', site 2: lo = 4.0 lies above hi = 3.5"),
    ({"a": [("moho", 0, 1)] * 60, "b": [("moho", 0, 1)] * 5}, 1, "class 'b': its term on 'moho' is the first beyond the 64"),
])
def test_check_classes_refuses(classes, S, text):
    with pytest.raises(ValueError, match=text):
        check_classes(classes, S, LABELS)


def test_check_classes_touches_no_engine():
    with pytest.raises(ValueError, match="none formed"):
        check_classes({"a": [("moho", 1, 2)]}, 1, {})
