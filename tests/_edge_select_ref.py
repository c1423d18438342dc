"""numpy fp64 restatement of csrc/edge_select.hip (include/mlgnn.h): the closed-form PCA of a pair of columns, scikit-
learn's ``scale(with_mean=False)`` and the shared noise vector, then the brute-force ``|x - y|`` estimator of
tests/_mi_ref.py with its ``m_i`` counts.  The sums are taken in the kernel's order (a lane adds its positions t, t + 256,
..., then the xor butterfly over the 64 lanes of a wave, then the four waves in wave order), products and sums round
separately as numpy's do: apart from ``hypot`` the two run the same IEEE operations.

It also holds the scikit-learn loop as the reference writes it (``valid_pca_mutual_info``, multiloader.py:828-874)."""
import numpy as np

from _mi_ref import mi_ref

BLOCK, WAVE = 256, 64
EPS = float(np.finfo(np.float64).eps)


def block_sum(v):
    """The sum of ``v [n]`` in the kernel's order."""
    v = np.asarray(v, dtype=np.float64)
    rows = -(-v.size // BLOCK)
    padded = np.zeros(rows * BLOCK)
    padded[:v.size] = v
    acc = np.zeros(BLOCK)
    for r in padded.reshape(rows, BLOCK):
        acc = acc + r                                              # (+ 0.0 for the lanes past the end: no rounding)
    lane = np.arange(BLOCK)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lane ^ o]
    return float(((acc[0] + acc[WAVE]) + acc[2 * WAVE]) + acc[3 * WAVE])


def leading_axis(a, b, c):
    """The leading eigenvector of ``[[a, b], [b, c]]``, its component of larger magnitude positive (the first on a tie)."""
    if b != 0.0:
        lam = (a + c) / 2.0 + np.hypot((a - c) / 2.0, b)
        u, w = (b, lam - a), (lam - c, b)
        nu, nw = np.hypot(*u), np.hypot(*w)
        v = (w[0] / nw, w[1] / nw) if nw > nu else (u[0] / nu, u[1] / nu)
    else:
        v = (1.0, 0.0) if a >= c else (0.0, 1.0)
    if (v[0] < 0.0) if abs(v[0]) >= abs(v[1]) else (v[1] < 0.0):
        v = (-v[0], -v[1])
    return v


def pair_score(x, y):
    n = float(x.size)
    dx, dy = x - block_sum(x) / n, y - block_sum(y) / n
    v = leading_axis(block_sum(dx * dx), block_sum(dx * dy), block_sum(dy * dy))
    return dx * v[0] + dy * v[1]


def prepare_column(score, noise):
    """``scale(with_mean=False)`` and the noise of ``mutual_info_classif`` on one column."""
    n = float(score.size)
    d = score - block_sum(score) / n
    sd = np.sqrt(block_sum(d * d) / n)
    if sd < 10 * EPS:
        sd = 1.0
    z = score / sd
    amp = 1e-10 * max(1.0, block_sum(np.abs(z)) / n)
    return z + amp * noise


def prepared_ref(values, pairs, noise):
    """values [n, n_nodes] -> the prepared columns [P, n] (row p: pair p; ``t = -1``: the column ``s`` alone)."""
    x = np.asarray(values, dtype=np.float64)
    out = np.empty((len(pairs), x.shape[0]))
    for p, (s, t) in enumerate(np.asarray(pairs).tolist()):
        score = x[:, s].copy() if t < 0 else pair_score(x[:, s], x[:, t])
        out[p] = prepare_column(score, noise)
    return out


def pair_mi_ref(values, y, pairs, k, noise):
    """-> (mi [P], m [P, n] int64 in sample order, prepared [P, n]).  Every label occurs more than once."""
    prepared = prepared_ref(values, pairs, noise)
    mi, m = mi_ref(prepared.T, y, k)
    return mi, m, prepared


def noise_of(random_state, n):
    from sklearn.utils import check_random_state
    return check_random_state(random_state).standard_normal(n)


def edge_select_ref(values, y, edge_index, threshold, k, random_state):
    """-> (keep [E], mi_pair [E], mi_node {node: value}) by the restatement."""
    ei = np.asarray(edge_index).reshape(2, -1)
    nodes = np.unique(ei)
    pairs = np.concatenate([ei.T, np.stack([nodes, np.full_like(nodes, -1)], axis=1)], axis=0)
    mi = pair_mi_ref(values, y, pairs, k, noise_of(random_state, np.asarray(values).shape[0]))[0]
    mi_pair, single = mi[:ei.shape[1]], dict(zip(nodes.tolist(), mi[ei.shape[1]:].tolist()))
    keep = np.array([mi_pair[e] > threshold * max(single[int(ei[0, e])], single[int(ei[1, e])]) for e in range(ei.shape[1])],
                    dtype=bool)
    return keep, mi_pair, single


def sklearn_loop(values, y, edge_index, threshold, k, random_state, mutual_classif=True):
    """``valid_pca_mutual_info`` per edge, as the reference writes it (the end-node values cached per node)."""
    from sklearn.decomposition import PCA
    from sklearn.feature_selection import mutual_info_classif, mutual_info_regression
    x = np.asarray(values, dtype=np.float64)
    ei = np.asarray(edge_index).reshape(2, -1)
    mutual_infos, keep, mi_pair = {}, [], []
    for s, t in ei.T.tolist():
        edge_data = x[:, [s, t]]
        pca = PCA(n_components=1)
        pca = pca.fit(edge_data)
        pca_data = pca.transform(edge_data)
        if mutual_classif:
            pca_mutual_info = mutual_info_classif(pca_data, y, n_neighbors=k, random_state=random_state)
        else:
            pca_mutual_info = mutual_info_regression(pca_data, y, n_neighbors=k)
        for v in (s, t):
            if v not in mutual_infos:
                fn = mutual_info_classif if mutual_classif else mutual_info_regression
                mutual_infos[v] = fn(x[:, v][:, None], y, n_neighbors=k, random_state=random_state)
        keep.append(bool(pca_mutual_info > threshold * max(mutual_infos[s], mutual_infos[t])))
        mi_pair.append(float(pca_mutual_info[0]))
    return np.array(keep, dtype=bool), np.array(mi_pair), {v: float(m[0]) for v, m in mutual_infos.items()}


def make_values(counts, n_nodes, seed, quantised=False):
    """``values [n, n_nodes]`` fp64 and ``y [n]`` with ``counts[l]`` samples of label ``l`` in a shuffled order.  A planted
    signal of varying strength in every column (column v is shifted by ``label * (1 + 2 v / n_nodes)``, so few
    estimates clamp to 0) and a shared factor, so that pairs are correlated.  ``quantised``: five levels per column."""
    rng = np.random.RandomState(seed)
    y = np.repeat(np.arange(len(counts)), counts)
    rng.shuffle(y)
    n = len(y)
    shared = rng.standard_normal((n, 1))
    x = rng.standard_normal((n, n_nodes)) + 0.6 * shared + y[:, None] * (1.0 + 2.0 * np.arange(n_nodes) / n_nodes)[None, :]
    if quantised:
        x = np.clip(np.round(x), -2, 2)
    return x, y.astype(np.int64)


def random_edges(n_nodes, n_edges, seed):
    """``[2, E]`` without self-loops: on ``(s, s)`` the pair's value equals the node's own up to rounding, so its
    decision always lies inside the margin."""
    rng = np.random.RandomState(seed)
    src = rng.randint(0, n_nodes, n_edges)
    return np.stack([src, (src + rng.randint(1, n_nodes, n_edges)) % n_nodes])
