"""The ``--knn_mutual_info`` form of the fold preparation's edge test on the kernel of csrc/kraskov_mi.hip: for a PPI edge
whose omics is not 1 the reference's ``valid_pca_mutual_info`` (``dataloader/multiloader.py:838-839, 853-854, 863-864``)
calls ``utils/knnie.py::kraskov_mi`` -- the Kraskov-Stoegbauer-Grassberger estimator on three KD-trees, ``k = 5`` -- on the
two RAW end columns against the label, and on each end column alone.  No PCA, no scaling and no noise, so the kernel's
distances and neighbour counts are the reference's exactly; only the order of the final sums differs.

:func:`kraskov_mi` is the op (one workgroup per pair, one launch), :func:`kraskov_mi_host` the reference's estimate from
the same ``scipy.spatial.cKDTree`` queries, and :func:`edge_select_knn` the decision: ONE launch over the ``E`` edges and
the ``U`` distinct end nodes, the comparison on the host in fp64.  The host leg runs where the kernel does not apply
(switch off, no GPU, more than 2048 patients, ``k > 16``, fewer than ``k + 1`` patients -- which it refuses, as the
reference does); it is the reference's arithmetic, not a stand-in for a missing kernel.

Where the ``(k + 1)``-th nearest distance of some sample is 0 (``k + 1`` coinciding samples) the reference takes
``log(0)`` and stops in its debugger trap.  The kernel reports NaN for that pair and the host function raises
``ValueError``; :func:`edge_select_knn` raises ``ValueError`` on either leg.

Allocation: every device output is ``torch.zeros`` (as in :mod:`mlgnn.pca`, for the reason its docstring gives); that the
kernel writes every output element whatever they held before is tested against the entry point directly
(tests/test_kraskov_gpu.py).  No gradient, no ``autograd.Function``."""
import os
from math import log

import numpy as np
import torch

from . import _lib, _pairs
from .mutual_info import MAX_SAMPLES

MAX_NEIGHBORS = 16          # MLGNN_KRASKOV_MAX_NEIGHBORS of include/mlgnn.h (tests/test_kraskov_abi.py compares)

# MLGNN_EDGE_KNN_FUSED=0: edge_select_knn always runs kraskov_mi_host (same-box A/B runs).  The default follows the
# measurement of tools/bench_edge_select_knn.py (profiles/edge_select_knn.json, README "Edge selection, k-NN form"): end
# to end the kernel leg beats the scaled host leg by far more than that leg's spread at the gbm and kirc shapes.
DEFAULT_ENABLED = True
ENABLED = os.environ.get("MLGNN_EDGE_KNN_FUSED", "1" if DEFAULT_ENABLED else "0") != "0"

# which leg edge_select_knn took.  A plain dict, not registered with _lib.stats, as for edge_select.EDGE_SELECT_STATS.
EDGE_KNN_STATS = {"hip": 0, "host": 0}


def kraskov_mi_supported(n, n_nodes, n_pairs, k=5, return_details=False):
    """Whether the kernel takes the shape: ``1 <= k <= 16``, ``k + 1 <= n <= 2048``, the arrays below 4 GiB.  The switch
    and the presence of a GPU are :func:`edge_select_knn`'s business."""
    k = int(k)
    if not 1 <= k <= MAX_NEIGHBORS:
        return False
    return bool(_lib.lib.mlgnn_kraskov_mi_supported(int(n), int(n_nodes), int(n_pairs), k, int(return_details)))


def kraskov_mi(values, y, pairs, k=5, return_details=False):
    """``kraskov_mi(values[:, [s, t]], y[:, None], k)`` of the reference for every row ``(s, t)`` of ``pairs [P, 2]``, and
    ``kraskov_mi(values[:, [s]], y[:, None], k)`` for a row ``(s, -1)`` -> fp64 numpy ``[P]``; NaN where the reference
    would take ``log(0)``.  ``values``: ``[n, n_nodes]`` fp32 or fp64 with any strides, on the host or the device (the
    upcast of fp32 is exact, so every form of the same values gives the same bits); ``y [n]``: any real column.
    ``return_details``: also ``kd [P, n]`` fp64 (the distance to the ``k + 1``-th nearest joint sample, self included),
    ``nx [P, n]`` and ``ny [P, n]`` int32 (the marginal counts inside ``kd - 1e-15``, self included)."""
    k = int(k)

    def prepare(label, n, n_nodes, n_pairs):
        from scipy.special import digamma
        if not kraskov_mi_supported(n, n_nodes, n_pairs, k, return_details):
            raise ValueError("kraskov_mi: unsupported shape (%d samples, %d nodes, %d pairs, k = %d; 1 <= k <= %d, "
                             "k + 1 <= n <= %d, below 4 GiB)" % (n, n_nodes, n_pairs, k, MAX_NEIGHBORS, MAX_SAMPLES))
        return (label,), digamma(k) + digamma(n), ()

    details = (torch.float64, torch.int32, torch.int32) if return_details else (None, None, None)
    return _pairs.pair_op("mlgnn.kraskov.kraskov_mi", "mlgnn_kraskov_mi", values, y, np.float64, pairs, prepare, details, k,
                          see="; see kraskov_mi_host")


def _ksg_on_trees(cols, label, k):
    """The KSG estimate of one pair on the host: ``cols [n, d]`` (``d`` = 2, or 1 for a single column), ``label [n, 1]``.
    The reference's quantities from the same scipy calls -- the Chebyshev distance to the ``k + 1``-th nearest joint
    sample (self included), the marginal neighbour counts inside that distance less 1e-15 -- each tree queried once for
    all samples, and its three entropy-like terms, log terms included, as means over the samples:

        h_joint = -psi(k) + psi(n) + (d + 1) log 2 + (d + 1) mean(log radius)
        h_cols  =           psi(n) +  d      log 2 +  d      mean(log radius) - mean(psi(n_cols))
        h_label =           psi(n) +         log 2 +         mean(log radius) - mean(psi(n_label))
        mi      = h_cols + h_label - h_joint"""
    from scipy.spatial import cKDTree
    from scipy.special import digamma
    n, d = cols.shape
    chebyshev = float("inf")
    joint = np.hstack([cols, label])
    radius = cKDTree(joint).query(joint, k + 1, p=chebyshev)[0][:, k]
    zero = int(np.count_nonzero(~(radius > 0)))
    if zero:
        raise ValueError("kraskov_mi_host: %d of %d samples have %d coinciding neighbours (kd = 0): the reference takes "
                         "log(0) here" % (zero, n, k))
    inside = radius - 1e-15
    n_cols = cKDTree(cols).query_ball_point(cols, inside, p=chebyshev, return_length=True)
    n_label = cKDTree(label).query_ball_point(label, inside, p=chebyshev, return_length=True)
    mean_log = np.log(radius).mean()
    h_joint = -digamma(k) + digamma(n) + (d + 1) * (log(2) + mean_log)
    h_cols = digamma(n) + d * (log(2) + mean_log) - digamma(n_cols).mean()
    h_label = digamma(n) + (log(2) + mean_log) - digamma(n_label).mean()
    return float(h_cols + h_label - h_joint)


def kraskov_mi_host(values, y, pairs, k=5):
    """:func:`kraskov_mi` as the reference computes it, on the host: per pair three ``scipy.spatial.cKDTree`` (joint, x,
    y), the ``k + 1`` query with ``p=inf``, ``query_ball_point`` at ``kd - 1e-15``, the three terms with their log parts
    (as means over the samples, where the reference adds sample by sample: another order of the same fp64 terms).
    Raises ``ValueError`` where some ``kd`` is 0, and for ``k > n - 1`` (the reference's assertion)."""
    x = _pairs.host(values).astype(np.float64, copy=False)
    if x.ndim != 2:
        raise ValueError("kraskov_mi_host: values must be [n, n_nodes]")
    label = np.ascontiguousarray(_pairs.host(y).reshape(-1), dtype=np.float64)[:, None]
    if label.shape[0] != x.shape[0]:
        raise ValueError("kraskov_mi_host: y has %d entries for %d samples" % (label.shape[0], x.shape[0]))
    p = _pairs.check_pairs(pairs, x.shape[1], "kraskov_mi")
    k = int(k)
    if not 1 <= k <= x.shape[0] - 1:
        raise ValueError("kraskov_mi_host: k = %d needs 1 <= k <= n - 1 = %d" % (k, x.shape[0] - 1))
    out = np.zeros(p.shape[0], dtype=np.float64)
    for e, (s, t) in enumerate(p.tolist()):
        out[e] = _ksg_on_trees(np.ascontiguousarray(x[:, [s, t] if t >= 0 else [s]]), label, k)
    return out


def use_kernel(n, n_nodes, n_edges, k):
    """:func:`edge_select_knn`'s dispatch rule: the kernel when ``MLGNN_EDGE_KNN_FUSED`` is on, a GPU is present and
    :func:`kraskov_mi_supported` holds for the ``E`` pairs and at most ``min(2 E, n_nodes)`` singles of the launch."""
    return bool(ENABLED and torch.cuda.is_available()) and kraskov_mi_supported(
        n, n_nodes, _pairs.kernel_budget(n_edges, n_nodes), k)


def edge_select_knn(values, y, edge_index, threshold=1.0, k=5):
    """``valid_pca_mutual_info`` under ``--knn_mutual_info`` for every edge of ``edge_index [2, E]`` (node indices into
    the columns of ``values [n, n_nodes]``, the training patients' rows) -> ``(keep [E] bool, mi_pair [E] fp64, mi_node
    {node: value})`` like :func:`mlgnn.edge_select.edge_select`: edge ``e`` is kept iff ``mi_pair[e] > threshold *
    max(mi_node[src], mi_node[dst])``, decided on the host in fp64.  On the kernel ONE launch covers the ``E`` pairs and
    the ``U`` distinct end nodes; otherwise :func:`kraskov_mi_host` runs on the same list.  ``ValueError`` where a pair
    or an end node has ``k + 1`` coinciding samples.  ``EDGE_KNN_STATS`` counts the leg."""
    ei, n, n_nodes, n_edges = _pairs.check_edges(values, edge_index, "edge_select_knn")
    nodes, pairs = _pairs.launch_list(ei)
    if use_kernel(n, n_nodes, n_edges, k):
        EDGE_KNN_STATS["hip"] += 1
        mi = kraskov_mi(values, y, pairs, k)
        bad = int(np.isnan(mi).sum())
        if bad:
            raise ValueError("edge_select_knn: %d of %d pairs and end nodes have %d coinciding samples (kd = 0): the "
                             "reference takes log(0) there" % (bad, len(pairs), int(k) + 1))
    else:
        EDGE_KNN_STATS["host"] += 1
        mi = kraskov_mi_host(values, y, pairs, k)
    return _pairs.decide(mi, nodes, ei, threshold)
