"""A pure-Python integer restatement of the evaluation kernel's counts (csrc/eval_metrics.hip), shared by the host and the
GPU tests of the evaluation pass, and the bound that ties ``num / den`` to scikit-learn's ``roc_auc_score``."""
import numpy as np

U = 2.0 ** -53


def auc_bound(n):
    """``(n + 8) 2^-53``: scikit-learn sums at most ``n + 1`` non-negative trapezoid terms, each carrying a handful of
    fp64 roundings, to a value of at most 1; the integer form adds the one rounding of its division."""
    return (n + 8) * U


def counts(scores, positive):
    """``(n, n_pos, n_correct, num, den)`` of one row: ``scores`` fp32 values, ``positive`` booleans.
    ``num = sum over negatives j of (2 #{positives with s > s_j} + #{positives with s == s_j})``, ``den = 2 P N_neg``;
    comparisons are those of the float values, so ``-0.0 == +0.0``.  Quadratic, exact."""
    s = [float(v) for v in np.asarray(scores, dtype=np.float32).reshape(-1)]
    t = [bool(v) for v in np.asarray(positive).reshape(-1)]
    assert len(s) == len(t)
    pos = sorted(v for v, lab in zip(s, t) if lab)
    num = 0
    for v, lab in zip(s, t):
        if lab:
            continue
        lo = np.searchsorted(pos, v, side="left")               # positives below v
        hi = np.searchsorted(pos, v, side="right")              # positives below or equal
        num += 2 * (len(pos) - int(hi)) + (int(hi) - int(lo))
    n, n_pos = len(s), len(pos)
    n_correct = sum((v > 0.5) == lab for v, lab in zip(s, t))
    return n, n_pos, n_correct, num, 2 * n_pos * (n - n_pos)


def make_scores(kind, n, rng):
    """fp32 scores of the four kinds the tests use."""
    if kind == "uniform":
        return rng.random(n, dtype=np.float32)
    if kind == "sevenths":                                       # heavy ties across both classes
        return (rng.integers(0, 8, n) / np.float32(7)).astype(np.float32)
    if kind == "equal":
        return np.full(n, 0.25, dtype=np.float32)
    if kind == "zeros":                                          # -0.0 and +0.0 among a few other values
        pool = np.array([-0.0, 0.0, -0.0, 0.0, 0.5, 0.75, 1.0], dtype=np.float32)
        s = pool[rng.integers(0, pool.size, n)]
        s[:2] = np.array([-0.0, 0.0], dtype=np.float32)[:n]
        return s
    raise KeyError(kind)


def make_labels(share, n, rng):
    """booleans with about ``share`` positives; both classes present once ``n >= 2`` and ``0 < share < 1``."""
    t = rng.random(n) < share
    if n >= 2 and 0.0 < share < 1.0:
        t[0], t[1] = True, False
    return t
