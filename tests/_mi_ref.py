"""numpy restatement of the mutual-information estimator of csrc/mutual_info.hip (include/mlgnn.h), an O(N^2) loop per
column on an already prepared fp64 array:

    k_i = min(k, count(d_i) - 1)
    r_i = the k_i-th smallest of fl|c_j - c_i| over j != i with d_j = d_i
    m_i = #{ j : fl|c_j - c_i| <= nextafter(r_i, 0) } over all samples, self included
    mi  = max(0, psi(N) + mean psi(k_i) - mean psi(count(d_i)) - mean psi(m_i))

after the samples whose label occurs once have been dropped (N counts the rest).  The last line is written with the
four terms in scikit-learn's order, so that where scikit-learn searches with its tree the values agree to the last bit."""
import numpy as np
from scipy.special import digamma


def keep_mask(y):
    y = np.asarray(y)
    _, inv, cnt = np.unique(y, return_inverse=True, return_counts=True)
    return cnt[inv] > 1


def mi_ref(prepared, y, k):
    """prepared [n, F] fp64, y [n] -> (mi [F] fp64, m [F, n_kept] int64 in the order of the kept samples)."""
    X = np.asarray(prepared, dtype=np.float64)
    y = np.asarray(y)
    keep = keep_mask(y)
    X, y = X[keep], y[keep]
    n, F = X.shape
    if n == 0:
        return np.zeros(F), np.zeros((F, 0), dtype=np.int64)
    _, d, cnt = np.unique(y, return_inverse=True, return_counts=True)
    count_i = cnt[d]
    k_i = np.minimum(k, count_i - 1)
    same = d[:, None] == d[None, :]
    np.fill_diagonal(same, False)
    mi = np.empty(F)
    m_all = np.empty((F, n), dtype=np.int64)
    for f in range(F):
        c = X[:, f]
        dist = np.abs(c[None, :] - c[:, None])                         # dist[i, j] = fl|c_j - c_i|
        own = np.where(same, dist, np.inf)
        own.sort(axis=1)
        r = own[np.arange(n), k_i - 1]
        m = (dist <= np.nextafter(r, 0)[:, None]).sum(axis=1)
        m_all[f] = m
        v = digamma(n) + np.mean(digamma(k_i)) - np.mean(digamma(count_i)) - np.mean(digamma(m))
        mi[f] = max(0, v)
    return mi, m_all


def make_input(counts, F, seed, halves=False):
    """Raw fp32 ``x [n, F]`` and int64 ``y [n]`` with ``counts[l]`` samples of label ``l`` in a shuffled order.  A planted
    signal: column f is shifted by ``label * 2 f / F``.  ``halves``: values rounded to multiples of 0.5 (heavy ties, which
    only the preparation's noise separates), column 0 constant and column 1 equal to the label."""
    rng = np.random.RandomState(seed)
    y = np.repeat(np.arange(len(counts)), counts)
    rng.shuffle(y)
    x = rng.standard_normal((len(y), F)) + y[:, None] * (2.0 * np.arange(F) / F)[None, :]
    if halves:
        x = np.round(x * 2.0) / 2.0
        x[:, 0] = 1.5
        if F > 1:
            x[:, 1] = y
    return x.astype(np.float32), y.astype(np.int64)
