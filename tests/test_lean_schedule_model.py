"""The schedule model of the trial-per-lane dispersion launch (tools/cpu_lean_schedule.py) and the pairing of swd_lean_kernel that it
restates, on 256 synthetic models; no GPU.

The fixture tests/golden/lean_rounds_256.npz holds the rounds this repository's oracle counts for them (search mode 2, the kernel's
window rule: `python tests/test_lean_schedule_model.py` writes it): it pins the rule, and the model's figures below rest on it."""
import os
import sys

import numpy as np

from conftest import REPO, GOLDEN

sys.path.insert(0, os.path.join(REPO, "tools"))
import cpu_lean_schedule as S  # noqa: E402
from bayhunter_amd.synth import synth_models, SWD_PERIODS  # noqa: E402

FIXTURE = os.path.join(GOLDEN, "lean_rounds_256.npz")
B, L = 256, 10


def models():
    return synth_models(np.random.RandomState(256), B, L, lvz_frac=0.1)


def test_the_oracle_counts_the_rounds_of_the_fixture(oracle):
    nlay, h, vp, vs, rho = models()
    g = np.load(FIXTURE, allow_pickle=False)
    for iwave, name in ((2, "rayleigh"), (1, "love")):
        rounds, steps = S.counted_rounds(nlay, h, vp, vs, rho, SWD_PERIODS, iwave)
        assert np.array_equal(rounds, g[name])
        # 30 periods: a round of clustered trials each, the first period's scan from cm, and a round for every 16 grid steps
        # beyond the 14 that ride along
        assert rounds.min() >= 31 and np.all(rounds <= 31 + np.ceil(np.maximum(steps, 0) / 16.0).sum(1))


def test_the_window_rule():
    steps = np.array([[15.0] + [13.0] * 3, [16.0] + [14.0, 29.0, 30.0], [40.0] + [-3.0, 0.0, 13.0]])
    # first period: start value + 15 steps in its first round; later periods: 13 steps inside the 14 lanes that rode along
    assert S.rounds_from_steps(steps).tolist() == [2 + 3, 3 + (2 + 2 + 3), 4 + 3]


def test_the_opposite_order_is_a_perfect_matching_of_opposite_ranks():
    """every Love group is taken once, and on every SIMD the two ranks add up to Q - 1 -- under the placement the pairing was
    written for: position q of both targets for the plain opposite order, the dispatcher's two passes for the pass-aware one"""
    for Q in (8, 16, 128):
        for H, place in ((0, "same"), (Q // 2, "rotate")):
            groups = [S.love_group(p, Q, H) for p in range(Q)]
            assert sorted(groups) == list(range(Q))
            pairs = S.placement_pairs(Q, place)
            assert sorted(q for q, _ in pairs) == list(range(Q)) and sorted(p for _, p in pairs) == list(range(Q))
            assert all(q + S.love_group(p, Q, H) == Q - 1 for q, p in pairs)
    # H that is not half of Q (not a launch of two workgroups per CU): the plain opposite order
    assert [S.love_group(p, 12, 4) for p in range(12)] == list(range(11, -1, -1))


def test_the_pass_aware_pairing_is_no_worse_on_the_fixture():
    """Under the placement the per-wavefront records show ("rotate") the pass-aware pairing is the one that pairs opposite ranks, so
    this compares it with the plain opposite order where it must win; under position-with-position placement the plain one wins
    likewise (profiles/lean_schedule_model.txt has both).  `love_group` restates the kernel's expression by hand: the check of the
    kernel's own mapping is tests/test_gpu_lean_schedule.py -- a mapping that is no permutation leaves rows unwritten and the bits
    differ from the order as given."""
    nlay, h, vp, vs, rho = models()
    g = np.load(FIXTURE, allow_pickle=False)
    key = S.key_range(nlay, h, vs)
    sb = S.block_sort(key)
    assert sorted(np.concatenate(sb).tolist()) == list(range(B))            # the order is a permutation ...
    assert all(np.all(s // (B // S.BLOCKS) == x) for x, s in enumerate(sb))  # ... and every model stays inside its block
    wR, wL = S.wave_rounds(sb, g["rayleigh"]), S.wave_rounds(sb, g["love"])
    Q = B // S.BLOCKS // S.MPW
    for solo in (0.5, 0.65):
        ends = {H: S.simd_ends(wR, wL, lambda q: S.placement_pairs(q, "rotate"), lambda p, q: S.love_group(p, q, H), solo) for H in (0, Q // 2)}
        assert ends[0].size == ends[Q // 2].size == S.BLOCKS * Q
        assert np.isclose(ends[0].mean(), ends[Q // 2].mean()) or solo != 0.5  # (the sum rule: the same work, shared out differently)
        assert ends[Q // 2].max() <= ends[0].max()


if __name__ == "__main__":
    nlay, h, vp, vs, rho = models()
    np.savez(FIXTURE, rayleigh=S.counted_rounds(nlay, h, vp, vs, rho, SWD_PERIODS, 2)[0].astype(np.int16),
             love=S.counted_rounds(nlay, h, vp, vs, rho, SWD_PERIODS, 1)[0].astype(np.int16))
