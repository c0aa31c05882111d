"""The host side of the credible intervals (bayhunter_amd/posterior.py: quantiles= of posterior_models, posterior_moho and
posterior_scalars): a bad quantile list is refused before any engine is touched, and the step from order-statistic keys to values
is numpy.quantile(..., method="linear") bit for bit."""
import numpy as np
import pytest

from bayhunter_amd import posterior as P


class Untouchable(object):
    """stands in for an engine: any use of it fails the test"""

    def __getattr__(self, name):
        raise AssertionError("the engine was touched (%s) before the quantiles were checked" % name)


ROWS = np.array([[3.0, 4.5, 0.0, 30.0], [3.2, 4.4, 0.0, 28.0]])
BAD = ([0.5, 1.5], [-0.1], [0.5, float("nan")], [0.5, "0.9"], [None], [0.5 + 0j], [[0.5]], 0.5, "0.5", [True])


def calls():
    eng = Untouchable()
    return (lambda q: P.posterior_models(ROWS, engine=eng, quantiles=q),
            lambda q: P.posterior_moho(ROWS, moho=(5.0, 40.0), engine=eng, quantiles=q),
            lambda q: P.posterior_scalars(ROWS, dict(like=np.zeros(2)), engine=eng, quantiles=q))


@pytest.mark.parametrize("bad", BAD, ids=[repr(b) for b in BAD])
def test_a_bad_quantile_list_is_a_value_error_before_the_gpu(bad):
    for call in calls():
        with pytest.raises(ValueError, match="quantiles"):
            call(bad)


def test_good_lists_keep_their_order_and_duplicates():
    q = P.check_quantiles((0.975, 0, 0.5, 0.5, 1, np.float32(0.25), np.int64(1)))
    assert q.dtype == np.float64 and np.array_equal(q, [0.975, 0.0, 0.5, 0.5, 1.0, 0.25, 1.0])
    assert P.check_quantiles(None) is None and P.check_quantiles(()).shape == (0,)
    assert np.array_equal(P.check_quantiles(np.array([0.1, 0.9])), [0.1, 0.9])


def okeys(v, k32):
    """the ordered keys of include/bh_engine_posterior.h of float64 values (k32: of their float32 bit patterns)"""
    if k32:
        u = np.asarray(v, np.float32).view(np.uint32)
        return np.where(u >> np.uint32(31), ~u, u | np.uint32(0x80000000)).astype(np.uint64)
    u = np.asarray(v, np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))


class FakeLoaded(object):
    """_Loaded's two key calls served from sorted host columns: what the kernels select, by definition"""

    def __init__(self, cols, k32):
        self.cols, self.k32 = cols, k32                # cols[s]: float64 [n_s, D]
        self.S = len(cols)
        self.rows = np.array([len(c) for c in cols], np.int64)

    def _pick(self, s, j, k):
        """the order statistics k and min(k + 1, n - 1) of column j of site s"""
        c = np.sort(self.cols[s][:, j])
        n = len(c)
        assert (n == 0 and k == 0) or k < n
        return None if n == 0 else (c[k], c[min(k + 1, n - 1)])

    def column_quantile_keys(self, dep, rank):                       # keys of the load's width, as the kernel gives them
        D, R = len(dep), rank.shape[1]
        assert 1 <= R <= 8 and rank.dtype == np.uint32
        lo, up = np.zeros((self.S, D, R), np.uint64), np.zeros((self.S, D, R), np.uint64)
        for s, j, r in np.ndindex(self.S, D, R):
            ab = self._pick(s, j, int(rank[s, r]))
            if ab is not None:
                lo[s, j, r], up[s, j, r] = okeys(ab[0], self.k32), okeys(ab[1], self.k32)
        return lo, up, self.k32

    def quantile_keys(self, which, rank):                            # 64-bit keys always (bh_posterior_scalar_quantiles)
        assert 1 <= rank.shape[2] <= 8
        lo, up = np.zeros(rank.shape, np.uint64), np.zeros(rank.shape, np.uint64)
        for s, j, r in np.ndindex(*rank.shape):
            ab = self._pick(s, j, int(rank[s, j, r]))
            if ab is not None:
                lo[s, j, r], up[s, j, r] = okeys(ab[0], False), okeys(ab[1], False)
        return lo, up


QS = (0.0, 0.025, 0.16, 1 / 3., 0.5, 0.5, 0.84, 0.975, 0.999, 1.0, 0.7)   # 11: a second call of 3, a duplicate, unsorted


@pytest.mark.parametrize("kind", ("f32", "f64"))
def test_keys_to_values_is_numpys_linear_quantile(kind):
    rs = np.random.RandomState(31)
    cols = []
    for n in (1, 2, 3, 8193, 0):
        c = rs.uniform(2.0, 4.8, (n, 3))
        c[:, 1] = np.round(c[:, 1] * 4) / 4                              # long runs of ties
        c[:, 2] = -c[:, 2]                                               # the other half of the key map
        c = c.astype(np.float32).astype(np.float64) if kind == "f32" else c + rs.uniform(-1e-9, 1e-9, c.shape)
        cols.append(c)
    if kind == "f64":
        assert any(np.any(c.astype(np.float32) != c) for c in cols)
    ld = FakeLoaded(cols, kind == "f32")
    got = P.column_quantiles(ld, np.arange(3.0), QS)                     # [S, R, D]
    gset = P.set_quantiles(ld, 0, np.repeat(ld.rows[:, None], 3, axis=1), QS)   # [S, Q, R]
    assert got.shape == (5, len(QS), 3) and gset.shape == (5, 3, len(QS))
    for s, c in enumerate(cols):
        if len(c) == 0:
            assert np.all(np.isnan(got[s])) and np.all(np.isnan(gset[s]))
            continue
        want = np.quantile(c, QS, axis=0, method="linear")
        assert np.array_equal(got[s].view(np.uint64), want.view(np.uint64)), (kind, len(c))
        assert np.array_equal(gset[s].T.copy().view(np.uint64), want.view(np.uint64)), (kind, len(c))
        for i, q in enumerate(QS):                                       # ... and the scalar formula, value by value
            k, g = P.quantile_rank(len(c), q)
            srt = np.sort(c[:, 0])
            v = P.quantile_lerp(srt[k], srt[min(k + 1, len(c) - 1)], g)
            assert np.float64(v).view(np.uint64) == want[i, 0].view(np.uint64)
