"""A plain restatement of the swap sweep of tempered chains (include/bh_engine_chain_ladder_sweep.h): one ladder at a time, one
pair at a time, in Python floats (IEEE doubles: every +, -, *, / below is one rounding, nothing is contracted).  The kernel is held
to these bits."""
import numpy as np

FLOOR = 2.0 ** -20          # 0x1p-20: the smallest gap an adaptation leaves, as a share of the ladder's span


def _div(a, b):
    """IEEE division (0/0 is NaN, x/0 is inf: no exception)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def adapted(b, wacc, wprop, kappa):
    """Step 3 for one ladder: b descending [R >= 3], the window counters of its R-1 pairs (all proposed).  Returns the new rung
    values, or None where they are not strictly decreasing."""
    R = len(b)
    A = [_div(float(int(wacc[i])), float(int(wprop[i]))) for i in range(R - 1)]
    s = 0.0
    for i in range(R - 1):
        s = s + A[i]
    abar = _div(s, float(R - 1))
    span = b[0] - b[R - 1]
    f = FLOOR * span
    g1 = []
    for i in range(R - 1):
        x = (b[i] - b[i + 1]) * (1.0 + kappa * (A[i] - abar))
        g1.append(x if x > f else f)
    s = 0.0
    for i in range(R - 1):
        s = s + g1[i]
    g2 = [_div(g1[i] * span, s) for i in range(R - 1)]
    nb = [b[0]]
    for r in range(1, R - 1):
        nb.append(nb[r - 1] - g2[r - 1])
    nb.append(b[R - 1])
    if all(nb[r] > nb[r + 1] for r in range(R - 1)):
        return nb
    return None


class SweepRef(object):
    """The plan: member lists and counters.  ladder[c] in 0..K-1, every id used."""

    def __init__(self, ladder):
        self.ladder = np.asarray(ladder, dtype=np.int64)
        self.C = self.ladder.size
        self.K = int(self.ladder.max()) + 1
        self.members = [np.flatnonzero(self.ladder == k) for k in range(self.K)]
        assert all(m.size for m in self.members)
        self.start = np.concatenate(([0], np.cumsum([m.size for m in self.members]))).astype(np.int64)
        self.proposed = np.zeros((2, self.C), dtype=np.int64)
        self.accepted = np.zeros((2, self.C), dtype=np.int64)
        self.wprop = np.zeros(self.C, dtype=np.int64)
        self.wacc = np.zeros(self.C, dtype=np.int64)
        self.adaptations = np.zeros(self.K, dtype=np.int64)
        self.skipped = np.zeros(self.K, dtype=np.int64)
        self.rung_beta = np.zeros(self.C)

    def sweep(self, like, beta, logu, parity, phase, adapt=0, kappa=0.0):
        """One sweep of every ladder: returns the new betas [C] (the inputs are left as they are)."""
        assert parity in (0, 1) and phase in (0, 1) and not (adapt and phase == 1)
        like, beta, logu = (np.asarray(a, dtype=np.float64) for a in (like, beta, logu))
        out = beta.copy()
        kappa = float(kappa)
        for k in range(self.K):
            idx, lo = self.members[k], int(self.start[k])
            R = idx.size
            order = idx[np.lexsort((idx, -beta[idx]))]
            b = [float(v) for v in beta[order]]
            l = [float(v) for v in like[order]]
            rung = list(range(R))                      # rung[p]: the rung chain order[p] holds after the swaps
            for r in range(parity, R - 1, 2):
                self.proposed[phase, lo + r] += 1
                self.wprop[lo + r] += 1
                if float(logu[lo + r]) < (b[r] - b[r + 1]) * (l[r + 1] - l[r]):
                    rung[r], rung[r + 1] = r + 1, r
                    self.accepted[phase, lo + r] += 1
                    self.wacc[lo + r] += 1
            final = b
            if adapt and R >= 3:
                nb = None
                if np.all(self.wprop[lo:lo + R - 1] > 0):
                    nb = adapted(b, self.wacc[lo:lo + R - 1], self.wprop[lo:lo + R - 1], kappa)
                if nb is None:
                    self.skipped[k] += 1
                else:
                    self.adaptations[k] += 1
                    final = nb
                self.wprop[lo:lo + R - 1] = 0
                self.wacc[lo:lo + R - 1] = 0
            for p in range(R):
                out[order[p]] = final[rung[p]]
            self.rung_beta[lo:lo + R] = final
        return out


def kappa_of(n, rate=0.5, lag=50.0):
    """the gain of adaptation number n (0 the first), as the host computes it"""
    return rate * lag / (n + lag)


def toy_sweep(ref, rs, beta, d, parity, phase, adapt=0, kappa=0.0):
    """One sweep of the idealised sampler: every chain's like is drawn afresh from its own temperature, like = -Gamma(d/2) / beta."""
    like = -rs.gamma(0.5 * d, size=beta.size) / beta
    logu = np.log(rs.uniform(size=beta.size))
    return ref.sweep(like, beta, logu, parity, phase, adapt, kappa)


def toy_run(b0, d, seed, windows, every, frozen, rate=0.5, lag=50.0):
    """`windows` adaptation windows of `every` sweeps from the ladder b0 (one ladder), then `frozen` sweeps that only count.
    Returns (final rung betas, rates of the frozen sweeps [R-1], the plan)."""
    rs = np.random.RandomState(seed)
    R = len(b0)
    ref = SweepRef(np.zeros(R, dtype=np.int64))
    beta = np.array(b0, dtype=np.float64)
    sweep = 0
    for n in range(windows):
        for j in range(every):
            last = j == every - 1
            beta = toy_sweep(ref, rs, beta, d, sweep % 2, 0, int(last), kappa_of(n, rate, lag) if last else 0.0)
            sweep += 1
    for _ in range(frozen):
        beta = toy_sweep(ref, rs, beta, d, sweep % 2, 1)
        sweep += 1
    with np.errstate(all="ignore"):
        rate_ = ref.accepted[1, :R - 1] / ref.proposed[1, :R - 1].astype(np.float64)
    return np.sort(beta)[::-1], rate_, ref
