"""numpy fp64 restatement of csrc/edge_select_cc.hip (include/mlgnn.h): the pair preparation of tests/_edge_select_ref.py
(closed-form PCA of two columns, ``scale(with_mean=False)``, the noise) followed by the brute-force Kraskov estimator of
tests/_mi_cc_ref.py with its ``nx_i`` and ``ny_i`` counts, against a target prepared as ``mutual_info_regression``
prepares it.

It also holds the scikit-learn loop as the reference writes it for ``mutual_classif`` false (``valid_pca_mutual_info``,
multiloader.py:828-874), with a ``random_state`` for the pair call as well (the reference passes none there)."""
import numpy as np

from _edge_select_ref import prepared_ref
from _mi_cc_ref import mi_cc_ref


def noises_of(random_state, y):
    """What one seeded ``mutual_info_regression`` call on a single feature draws and does to its target ->
    ``(noise_x [n], y_prepared [n])``: ``n`` normals for the feature first, then ``n`` for the target."""
    from sklearn.preprocessing import scale
    from sklearn.utils import check_random_state
    y = np.asarray(y, dtype=np.float64)
    rng = check_random_state(random_state)
    noise_x = rng.standard_normal(y.size)
    yp = scale(y, with_mean=False)
    return noise_x, yp + 1e-10 * np.maximum(1, np.mean(np.abs(yp))) * rng.standard_normal(y.size)


def pair_mi_reg_ref(values, y_prepared, pairs, k, noise_x, prepared=None):
    """-> (mi [P], nx [P, n], ny [P, n] int64 in sample order, prepared [P, n]).  ``prepared``: the columns to run the
    estimator on instead of the restatement's own (the kernel's, for the comparison of the counts)."""
    if prepared is None:
        prepared = prepared_ref(values, pairs, noise_x)
    mi, nx, ny = mi_cc_ref(np.asarray(prepared).T, y_prepared, k)
    return mi, nx, ny, prepared


def _decide(ei, mi_pair, single, threshold):
    return np.array([mi_pair[e] > threshold * max(single[int(ei[0, e])], single[int(ei[1, e])])
                     for e in range(ei.shape[1])], dtype=bool)


def edge_select_reg_ref(values, y, edge_index, threshold, k, random_state, pair_random_state):
    """-> (keep [E], mi_pair [E], mi_node {node: value}) by the restatement; both states are seeds."""
    ei = np.asarray(edge_index).reshape(2, -1)
    nodes = np.unique(ei)
    noise_x, yp = noises_of(pair_random_state, y)
    mi_pair = pair_mi_reg_ref(values, yp, ei.T, k, noise_x)[0]
    noise_x, yp = noises_of(random_state, y)
    mi_single = pair_mi_reg_ref(values, yp, np.stack([nodes, np.full_like(nodes, -1)], axis=1), k, noise_x)[0]
    single = dict(zip(nodes.tolist(), mi_single.tolist()))
    return _decide(ei, mi_pair, single, threshold), mi_pair, single


def sklearn_loop_reg(values, y, edge_index, threshold, k, random_state, pair_random_state=None):
    """``valid_pca_mutual_info`` per edge with ``mutual_classif`` false, as the reference writes it (the end-node values
    cached per node); ``pair_random_state`` goes to the pair call, where the reference passes none."""
    from sklearn.decomposition import PCA
    from sklearn.feature_selection import mutual_info_regression
    x = np.asarray(values, dtype=np.float64)
    ei = np.asarray(edge_index).reshape(2, -1)
    mutual_infos, keep, mi_pair = {}, [], []
    for s, t in ei.T.tolist():
        edge_data = x[:, [s, t]]
        pca = PCA(n_components=1)
        pca = pca.fit(edge_data)
        pca_data = pca.transform(edge_data)
        pca_mutual_info = mutual_info_regression(pca_data, y, n_neighbors=k, random_state=pair_random_state)
        for v in (s, t):
            if v not in mutual_infos:
                mutual_infos[v] = mutual_info_regression(x[:, v][:, None], y, n_neighbors=k, random_state=random_state)
        keep.append(bool(pca_mutual_info > threshold * max(mutual_infos[s], mutual_infos[t])))
        mi_pair.append(float(pca_mutual_info[0]))
    return np.array(keep, dtype=bool), np.array(mi_pair), {v: float(m[0]) for v, m in mutual_infos.items()}
