"""check_features (bayhunter_amd/posterior.py): the host code that turns the user's dict of features into the kind list and the
[S][F][3] parameter table of bh_posterior_features.  No engine, no GPU."""
import re

import numpy as np
import pytest

from conftest import REPO
from bayhunter_amd import engine as E
from bayhunter_amd.posterior import FEATURE_COLS, FEATURE_KINDS, check_features

EVERY = dict(upper=("vsmean", 0, 15), vs30=("vstime", 0, 0.03), sed_t=("tts", 0, 2.5, ), slow=("vsmin", 0, 60), fast=("vsmax", 5, 60),
             lvz=("drop", 10, 80, 0.2), step=("jump", 20, 60), sediment=("above", 0, 10, 2.9), crustal=("nifaces", 0, 40))


def test_every_kind_gives_its_columns_and_labels():
    kinds, par, labels = check_features(EVERY, 3)
    assert kinds.dtype == np.int32 and par.dtype == np.float64 and par.shape == (3, 9, 3)
    assert [FEATURE_KINDS[k] for k in kinds] == [v[0] for v in EVERY.values()] == list(FEATURE_KINDS)
    assert list(kinds) == list(range(9))
    assert labels == ["upper", "vs30", "sed_t", "slow.value", "slow.depth", "fast.value", "fast.depth", "lvz.depth", "lvz.jump",
                      "step.depth", "step.jump", "sediment", "crustal"]
    assert len(labels) == sum(FEATURE_COLS[k] for k in FEATURE_KINDS) == 13
    for s in range(3):
        assert np.array_equal(par[s, 5], [10, 80, 0.2]) and np.array_equal(par[s, 6], [20, 60, 0.0])     # c defaults to 0
        assert np.array_equal(par[s, 7], [0, 10, 2.9]) and np.array_equal(par[s, 1], [0, 0.03, 0.0])


def test_the_constants_mirror_the_header():
    txt = open(REPO + "/include/bh_engine_posterior_features.h").read()
    defs = {k: int(v) for k, v in re.findall(r"^#define\s+(BH_[A-Z0-9_]+)\s+(-?\d+)\b", txt, flags=re.M)}
    assert defs["BH_SCALARS_FEATURES"] == E.SCALARS_FEATURES == 4 and defs["BH_FEATURES_MAXKINDS"] == E.FEATURES_MAXKINDS == 64
    for i, k in enumerate(FEATURE_KINDS):
        assert defs["BH_FEATURE_" + k.upper()] == getattr(E, "FEATURE_" + k.upper()) == i
    sc = open(REPO + "/include/bh_engine_posterior_scalars.h").read()
    assert int(re.search(r"#define\s+BH_SCALARS_MAXCOLS\s+(\d+)", sc).group(1)) == E.SCALARS_MAXCOLS
    body = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert sorted(set(re.findall(r"\b(bh_[a-z_0-9]+)\s*\(", body))) == sorted(E.POSTERIOR_FEATURES_SYMBOLS)


def test_numbers_are_one_value_or_one_per_site():
    kinds, par, labels = check_features(dict(lvz=("drop", [5, 10, 15], 80.0, np.array([0.1, 0.2, 0.3])), m=("vsmean", 0, (20, 30, 40))), 3)
    assert np.array_equal(par[:, 0], [[5, 80, 0.1], [10, 80, 0.2], [15, 80, 0.3]])
    assert np.array_equal(par[:, 1], [[0, 20, 0], [0, 30, 0], [0, 40, 0]])
    assert labels == ["lvz.depth", "lvz.jump", "m"]
    for bad in ([5, 10], [5, 10, 15, 20], [[5, 10, 15]], []):
        with pytest.raises(ValueError, match="'lvz'.*z0"):
            check_features(dict(ok=("tts", 0, 1), lvz=("drop", bad, 80.0)), 3)
    with pytest.raises(ValueError, match="'m'.*z1"):
        check_features(dict(m=("vsmean", 0, (20, 30))), 3)
    with pytest.raises(ValueError, match="'a'.*c must be"):
        check_features(dict(a=("above", 0, 10, [3.0, 3.1])), 3)
    with pytest.raises(ValueError, match="'a'.*z0"):
        check_features(dict(a=("above", "deep", 10, 3.0)), 1)


@pytest.mark.parametrize("spec, msg", [
    (("vsmedian", 0, 10), "'f'.*unknown kind 'vsmedian'"),
    ((3, 0, 10), "'f'.*unknown kind"),
    (("vsmean", 0), "'f'.*expected"),
    (("drop", 0, 10, 0.1, 7), "'f'.*expected"),
    ("vsmean", "'f'.*expected"),
    (("vsmean", 0, 10, 1.0), "'f'.*takes no c"),
    (("above", 0, 10), "'f'.*needs c"),
    (("vsmean", -1.0, 10), "'f', site 0.*below 0"),
    (("vsmean", 10, 10), "'f', site 0.*z0 < z1"),
    (("tts", 10, 5), "'f', site 0.*z0 < z1"),
    (("vsmean", 0, np.inf), "'f', site 0.*finite"),
    (("vsmean", np.nan, 10), "'f', site 0.*finite"),
    (("above", 0, 10, np.nan), "'f', site 0.*finite"),
    (("drop", 0, 10, -0.1), "'f', site 0.*negative"),
    (("jump", 0, 10, -1e-300), "'f', site 0.*negative"),
])
def test_every_refusal_names_the_feature(spec, msg):
    with pytest.raises(ValueError, match=msg):
        check_features(dict(fine=("nifaces", 0, 10), f=spec), 2)


def test_a_refusal_names_the_site_at_fault():
    with pytest.raises(ValueError, match="'w', site 2.*z0 < z1"):
        check_features(dict(w=("vsmax", [0, 5, 30], [10, 20, 30])), 3)
    with pytest.raises(ValueError, match="'lvz', site 1.*negative"):
        check_features(dict(lvz=("drop", 0, 50, [0.0, -0.5])), 2)
    assert check_features(dict(a=("above", 0, 10, -1.0)), 1)[1][0, 0, 2] == -1.0     # above's c is a velocity: any finite number


def test_too_many_features_columns_and_bad_names():
    many = {"f%d" % i: ("nifaces", 0, 10 + i) for i in range(64)}
    assert len(check_features(many, 1)[2]) == 64
    with pytest.raises(ValueError, match="65 features"):
        check_features(dict(many, extra=("tts", 0, 1)), 1)
    two = {"d%d" % i: ("drop", 0, 10 + i) for i in range(32)}
    assert len(check_features(two, 1)[2]) == 64
    with pytest.raises(ValueError, match="65 columns.*'last'"):
        check_features(dict(two, last=("tts", 0, 1)), 1)
    for bad in ({}, None, [("vsmean", 0, 1)]):
        with pytest.raises(ValueError, match="features must be a dict"):
            check_features(bad, 1)
    for name in ("rows", "invalid_rows", "dropped"):
        with pytest.raises(ValueError, match="%r.*key of the result" % name):
            check_features({name: ("tts", 0, 1)}, 1)
    with pytest.raises(ValueError, match="name must be"):
        check_features({3: ("tts", 0, 1)}, 1)
