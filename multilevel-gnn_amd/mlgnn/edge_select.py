"""The ``--edge_select`` test of the fold preparation on the kernel of csrc/edge_select.hip: the reference's
``valid_pca_mutual_info`` (``dataloader/multiloader.py:828-874``) keeps a PPI edge iff the mutual information between the
label and the first principal component of its two end columns exceeds ``edge_select_threshold`` times the larger of the
two end columns' own -- three scikit-learn calls per edge, tens of thousands of edges per fold.  Here ONE launch computes
all of them: one workgroup per pair, ``E`` edges followed by the ``U`` distinct end nodes as single columns.

With a fixed ``random_state`` every ``mutual_info_classif`` call of the reference seeds a fresh generator, so every call
adds the same ``n`` noise values to its single column: one noise vector per fold, drawn on the host, is exactly what
scikit-learn does.  ``base``, ``psi``, the dense labels and the label drop are prepared as :func:`mlgnn.mutual_info.
mutual_info_cd` prepares them.

:func:`edge_select` runs the reference's own loop of scikit-learn calls on the host where the kernel does not apply
(switch off, no GPU, ``mutual_classif`` false, a label that occurs once, small classes, more than 2048 patients); that
leg is the reference's arithmetic, not a stand-in for a missing kernel.  The fold preparation sends ``mutual_classif`` false
to :func:`mlgnn.edge_select_reg.edge_select_regression` instead, which has a kernel of its own.

Allocation: every device output is ``torch.zeros`` (as in :mod:`mlgnn.pca`, for the reason its docstring gives); that the
kernel writes every output element whatever they held before is tested against the entry point directly
(tests/test_edge_select_gpu.py).  No gradient, no ``autograd.Function``."""
import os

import numpy as np
import torch

from . import _lib, _pairs
from .mutual_info import MAX_SAMPLES, tree_path

# MLGNN_EDGE_SELECT_FUSED=0: edge_select always runs the loop of scikit-learn calls (same-box A/B runs).  The default
# follows the measurement of tools/bench_edge_select.py (profiles/edge_select.json, README "Edge selection"): end to end
# the kernel leg beats the scikit-learn leg by far more than that leg's spread at the gbm and kirc shapes.
DEFAULT_ENABLED = True
ENABLED = os.environ.get("MLGNN_EDGE_SELECT_FUSED", "1" if DEFAULT_ENABLED else "0") != "0"

# which leg edge_select took.  A plain dict, not registered with _lib.stats: the names of the MLGNN_PRINT_STATS report are
# pinned (tests/test_binding_host.py), as for pca.PCA_STATS.
EDGE_SELECT_STATS = {"hip": 0, "sklearn": 0}


def _labels(y):
    _, dense, counts = np.unique(_pairs.host(y).reshape(-1), return_inverse=True, return_counts=True)
    return dense, counts


def edge_select_supported(n, n_nodes, n_pairs, n_neighbors, counts_per_label, mutual_classif=True, return_scores=False):
    """Whether the kernel applies to ``n`` patients with ``counts_per_label``: ``mutual_classif`` true, every label
    occurring more than once (scikit-learn drops the samples of a unique label AFTER its preparation, which the kernel
    does not imitate), :func:`mlgnn.mutual_info.tree_path`, ``2 <= n <= 2048``, ``n_neighbors >= 1``, the arrays below
    4 GiB.  The switch and the presence of a GPU are :func:`edge_select`'s business."""
    counts = [int(c) for c in counts_per_label]
    k = int(n_neighbors)
    if not mutual_classif or not counts or min(counts) < 2 or sum(counts) != int(n) or not 1 <= k < 1 << 31:
        return False
    if not tree_path(k, counts) or int(n) > MAX_SAMPLES:
        return False
    return bool(_lib.lib.mlgnn_edge_mi_supported(int(n), int(n_nodes), int(n_pairs), k, len(counts), int(return_scores)))


def pair_mutual_info(values, y, pairs, n_neighbors=3, random_state=None, return_scores=False, return_counts=False):
    """``mutual_info_classif(PCA(n_components=1).fit_transform(values[:, [s, t]]), y, n_neighbors=..., random_state=...)``
    for every row ``(s, t)`` of ``pairs [P, 2]``, and ``mutual_info_classif(values[:, [s]], y, ...)`` for a row
    ``(s, -1)`` -> fp64 numpy ``[P]``.  ``values``: ``[n, n_nodes]`` fp32 or fp64 with any strides, on the host or the
    device (the upcast of fp32 is exact, so every form of the same values gives the same bits).  The noise is
    ``check_random_state(random_state).standard_normal(n)``, drawn on the host, the same for every pair.
    ``return_scores``: also the prepared columns ``[P, n]`` as handed to the estimator; ``return_counts``: also ``m_i``
    as int32 ``[P, n]`` in sample order.  The values are scikit-learn's where :func:`edge_select_supported` holds; the
    caller checks that first."""
    k = int(n_neighbors)

    def prepare(y, n, n_nodes, n_pairs):
        from scipy.special import digamma
        from sklearn.utils import check_random_state
        dense, count = _labels(y)
        noise = check_random_state(random_state).standard_normal(n)
        if count.min() < 2:
            raise ValueError("pair_mutual_info: a label occurs once (scikit-learn drops such samples after its "
                             "preparation; the kernel does not imitate that)")
        if not _lib.lib.mlgnn_edge_mi_supported(n, n_nodes, n_pairs, k if -(1 << 31) <= k < 1 << 31 else 0, len(count),
                                                int(return_scores)):
            raise ValueError("pair_mutual_info: unsupported shape (%d samples, %d nodes, %d pairs, k = %d; 2 <= n <= %d, "
                             "k >= 1, below 4 GiB)" % (n, n_nodes, n_pairs, k, MAX_SAMPLES))
        count_i = count[dense]
        base = digamma(n) + np.mean(digamma(np.minimum(k, count_i - 1))) - np.mean(digamma(count_i))
        return (noise, dense.astype(np.int32)), base, (len(count),)

    return _pairs.pair_op("mlgnn.edge_select.pair_mutual_info", "mlgnn_edge_mi", values, y, None, pairs, prepare,
                          (torch.float64 if return_scores else None, torch.int32 if return_counts else None), k)


def sklearn_edge_select(values, y, edge_index, threshold=1.0, n_neighbors=3, random_state=None, mutual_classif=True,
                        pair_random_state=None):
    """The reference's loop (``valid_pca_mutual_info``), call for call: per edge ``PCA(n_components=1)`` on the two end
    columns and the mutual information of its score, the end columns' own cached per node.  As in the reference the
    regression path's pair call passes no ``random_state``: it takes ``pair_random_state``, whose default is the
    reference's.  (``n_neighbors`` is the reference's default of 3 there.)"""
    from sklearn.decomposition import PCA
    from sklearn.feature_selection import mutual_info_classif, mutual_info_regression
    x = _pairs.host(values).astype(np.float64, copy=False)
    y = _pairs.host(y).reshape(-1)
    ei = _pairs.host(edge_index).reshape(2, -1)
    keep = np.zeros(ei.shape[1], dtype=bool)
    mi_pair = np.zeros(ei.shape[1], dtype=np.float64)
    mi_node = {}

    def node(v):
        if v not in mi_node:
            fn = mutual_info_classif if mutual_classif else mutual_info_regression
            mi_node[v] = float(fn(x[:, v][:, None], y, n_neighbors=n_neighbors, random_state=random_state)[0])
        return mi_node[v]

    for e in range(ei.shape[1]):
        s, t = int(ei[0, e]), int(ei[1, e])
        edge_data = x[:, [s, t]]
        pca_data = PCA(n_components=1).fit(edge_data).transform(edge_data)
        if mutual_classif:
            mi_pair[e] = mutual_info_classif(pca_data, y, n_neighbors=n_neighbors, random_state=random_state)[0]
        else:
            mi_pair[e] = mutual_info_regression(pca_data, y, n_neighbors=n_neighbors, random_state=pair_random_state)[0]
        keep[e] = mi_pair[e] > threshold * max(node(s), node(t))
    return keep, mi_pair, mi_node


def use_kernel(n, n_nodes, n_edges, n_neighbors, counts_per_label, mutual_classif):
    """:func:`edge_select`'s dispatch rule: the kernel when ``MLGNN_EDGE_SELECT_FUSED`` is on, a GPU is present and
    :func:`edge_select_supported` holds for the ``E`` pairs and at most ``min(2 E, n_nodes)`` singles of the launch."""
    return bool(ENABLED and torch.cuda.is_available()) and edge_select_supported(
        n, n_nodes, _pairs.kernel_budget(n_edges, n_nodes), n_neighbors, counts_per_label, mutual_classif)


def edge_select(values, y, edge_index, threshold=1.0, n_neighbors=3, random_state=None, mutual_classif=True,
                knn_mutual_info=False):
    """``valid_pca_mutual_info`` for every edge of ``edge_index [2, E]`` (node indices into the columns of ``values
    [n, n_nodes]``, the training patients' rows) -> ``(keep [E] bool, mi_pair [E] fp64, mi_node {node: value})``: edge
    ``e`` is kept iff ``mi_pair[e] > threshold * max(mi_node[src], mi_node[dst])``, decided on the host in fp64.  On the
    kernel ONE launch covers the ``E`` pairs and the ``U`` distinct end nodes; otherwise the loop of scikit-learn calls
    runs (it also serves ``mutual_classif=False``).  With ``random_state=None`` the kernel leg draws one unseeded noise
    vector per call where the reference draws one per scikit-learn call.  ``EDGE_SELECT_STATS`` counts the leg."""
    if knn_mutual_info:
        raise NotImplementedError("knn_mutual_info (the reference's kraskov_mi) is not served by edge_select: call "
                                  "mlgnn.kraskov.edge_select_knn for the edges whose omics is not 1")
    ei, n, n_nodes, n_edges = _pairs.check_edges(values, edge_index, "edge_select")
    if use_kernel(n, n_nodes, n_edges, n_neighbors, _labels(y)[1], mutual_classif):
        EDGE_SELECT_STATS["hip"] += 1
        nodes, pairs = _pairs.launch_list(ei)
        return _pairs.decide(pair_mutual_info(values, y, pairs, n_neighbors, random_state), nodes, ei, threshold)
    EDGE_SELECT_STATS["sklearn"] += 1
    return sklearn_edge_select(values, y, ei, threshold, n_neighbors, random_state, mutual_classif)
