"""A numpy brute-force restatement of the kernel of csrc/kraskov_mi.hip (the reference's ``utils/knnie.py::kraskov_mi``
with its three KD-trees replaced by full distance matrices), shared by tests/test_kraskov_host.py and
tests/test_kraskov_gpu.py.

Per pair: the Chebyshev distance matrices of the x block and of y, ``kd = np.sort(max(dx, dy), axis=1)[:, k]`` (self and
duplicates included), the two counts at ``kd - 1e-15`` (one fp64 subtraction, self included) and the closed form
``psi(k) + psi(n) - mean psi(nx) - mean psi(ny)``: the reference's three sums of ``log kd`` cancel identically.  A pair
with a zero ``kd`` gets NaN, where the reference takes ``log(0)``."""
import numpy as np
from scipy.special import digamma


def details_ref(x, y, k):
    """``(kd [n] fp64, nx [n], ny [n])`` of one pair: ``x [n, d_x]``, ``y [n]``."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    dx = np.abs(x[:, None, :] - x[None, :, :]).max(axis=2)
    dy = np.abs(y[:, None] - y[None, :])
    kd = np.sort(np.maximum(dx, dy), axis=1)[:, k]
    r = kd - 1e-15
    nx = (dx <= r[:, None]).sum(axis=1)
    ny = (dy <= r[:, None]).sum(axis=1)
    return kd, nx.astype(np.int64), ny.astype(np.int64)


def kraskov_ref(values, y, pairs, k):
    """``(mi [P], kd [P, n], nx [P, n], ny [P, n])`` for the rows ``(s, t)`` of ``pairs`` (``t < 0``: column ``s`` alone)."""
    values = np.asarray(values, dtype=np.float64)
    n = values.shape[0]
    pairs = np.asarray(pairs).reshape(-1, 2)
    mi = np.zeros(len(pairs))
    kd = np.zeros((len(pairs), n))
    nx = np.zeros((len(pairs), n), dtype=np.int64)
    ny = np.zeros((len(pairs), n), dtype=np.int64)
    for e, (s, t) in enumerate(pairs.tolist()):
        kd[e], nx[e], ny[e] = details_ref(values[:, [s, t] if t >= 0 else [s]], y, k)
        if (kd[e] > 0).all():
            mi[e] = digamma(k) + digamma(n) - digamma(nx[e]).mean() - digamma(ny[e]).mean()
        else:
            mi[e] = np.nan
    return mi, kd, nx, ny


def tree_details(x, y, k):
    """The same three arrays from the scipy calls the reference makes, one sample at a time: the ``k + 1`` query on the
    joint tree with ``p=inf``, ``query_ball_point`` at ``kd - 1e-15`` on the tree of ``x`` and on the tree of ``y``."""
    from scipy.spatial import cKDTree
    cols = np.asarray(x, dtype=np.float64)
    label = np.asarray(y, dtype=np.float64).reshape(-1, 1)
    joint = np.hstack([cols, label])
    trees = {"joint": cKDTree(joint), "cols": cKDTree(cols), "label": cKDTree(label)}
    n = len(cols)
    kd = np.zeros(n)
    nx = np.zeros(n, dtype=np.int64)
    ny = np.zeros(n, dtype=np.int64)
    for i in range(n):
        kd[i] = trees["joint"].query(joint[i], k + 1, p=np.inf)[0][k]
        nx[i] = len(trees["cols"].query_ball_point(cols[i], kd[i] - 1e-15, p=np.inf))
        ny[i] = len(trees["label"].query_ball_point(label[i], kd[i] - 1e-15, p=np.inf))
    return kd, nx, ny


def columns(kind, n, n_nodes, seed):
    """``(values [n, n_nodes], y [n])`` of one input kind: ``continuous``; ``integer``: integer-valued columns scaled by
    100, where ``kd - 1e-15`` rounds back to ``kd`` (boundary points are counted); ``quarter``: quarter-step quantised
    columns, where it does not (they are excluded).  ``y`` is a 0/1 label except for ``continuous``, which draws it."""
    rng = np.random.RandomState(seed)
    if kind == "continuous":
        return rng.standard_normal((n, n_nodes)), rng.standard_normal(n)
    label = (rng.rand(n) < 0.4).astype(np.float64)
    if kind == "integer":
        return 100.0 * rng.randint(-6, 7, size=(n, n_nodes)).astype(np.float64), 100.0 * label
    if kind == "quarter":
        return np.round(4.0 * rng.standard_normal((n, n_nodes))) / 4.0, label
    raise ValueError(kind)


def cohort(n, n_nodes, n_edges, seed):
    """A small fold for the decision tests: continuous columns carrying the 0/1 label with a strength of their own, a
    label column and ``[2, n_edges]`` random edges without self-loops."""
    rng = np.random.RandomState(seed)
    label = (rng.rand(n) < 0.5).astype(np.float64)
    strength = rng.uniform(0.0, 2.5, size=n_nodes)
    values = rng.standard_normal((n, n_nodes)) + label[:, None] * strength[None, :]
    src = rng.randint(0, n_nodes, n_edges)
    dst = (src + rng.randint(1, n_nodes, n_edges)) % n_nodes
    return values, label, np.stack([src, dst])
