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

from . import _lib
from .mutual_info import MAX_SAMPLES, tree_path

# MLGNN_EDGE_SELECT_FUSED=0: edge_select always runs the loop of scikit-learn calls (same-box A/B runs).  The default
# follows the measurement of tools/bench_edge_select.py (profiles/edge_select.json, README "Edge selection"): end to end
# the kernel leg beats the scikit-learn leg by far more than that leg's spread at the gbm and kirc shapes.
DEFAULT_ENABLED = True
ENABLED = os.environ.get("MLGNN_EDGE_SELECT_FUSED", "1" if DEFAULT_ENABLED else "0") != "0"

# which leg edge_select took.  A plain dict, not registered with _lib.stats: the names of the MLGNN_PRINT_STATS report are
# pinned (tests/test_binding_host.py), as for pca.PCA_STATS.
EDGE_SELECT_STATS = {"hip": 0, "sklearn": 0}


def _host(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def _labels(y):
    y = _host(y).reshape(-1)
    _, dense, counts = np.unique(y, return_inverse=True, return_counts=True)
    return y, dense, counts


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


def _check_pairs(pairs, n_nodes):
    p = _host(pairs)
    if p.size == 0:
        p = p.reshape(0, 2)
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError("pair_mutual_info: pairs must be [P, 2], got %s" % (p.shape,))
    p = np.ascontiguousarray(p, dtype=np.int64)
    if p.shape[0] and (p[:, 0].min() < 0 or p[:, 0].max() >= n_nodes or p[:, 1].min() < -1 or p[:, 1].max() >= n_nodes):
        raise ValueError("pair_mutual_info: node indices outside [0, %d) (-1 in column 1: a single column)" % n_nodes)
    return p


def pair_mutual_info(values, y, pairs, n_neighbors=3, random_state=None, return_scores=False, return_counts=False):
    """``mutual_info_classif(PCA(n_components=1).fit_transform(values[:, [s, t]]), y, n_neighbors=..., random_state=...)``
    for every row ``(s, t)`` of ``pairs [P, 2]``, and ``mutual_info_classif(values[:, [s]], y, ...)`` for a row
    ``(s, -1)`` -> fp64 numpy ``[P]``.  ``values``: ``[n, n_nodes]`` fp32 or fp64 with any strides, on the host or the
    device (the upcast of fp32 is exact, so every form of the same values gives the same bits).  The noise is
    ``check_random_state(random_state).standard_normal(n)``, drawn on the host, the same for every pair.
    ``return_scores``: also the prepared columns ``[P, n]`` as handed to the estimator; ``return_counts``: also ``m_i``
    as int32 ``[P, n]`` in sample order.  The values are scikit-learn's where :func:`edge_select_supported` holds; the
    caller checks that first."""
    from scipy.special import digamma
    from sklearn.utils import check_random_state
    x = values if torch.is_tensor(values) else torch.from_numpy(np.asarray(values))
    if x.dim() != 2 or x.dtype not in (torch.float32, torch.float64):
        raise ValueError("pair_mutual_info: values must be [n, n_nodes] fp32 or fp64, got %s %s" % (tuple(x.shape), x.dtype))
    n, n_nodes = int(x.shape[0]), int(x.shape[1])
    y, dense, count = _labels(y)
    if y.shape != (n,):
        raise ValueError("pair_mutual_info: y has %d entries for %d samples" % (y.size, n))
    p = _check_pairs(pairs, n_nodes)
    n_pairs, k = int(p.shape[0]), int(n_neighbors)
    noise = check_random_state(random_state).standard_normal(n)       # (drawn whatever P is: the generator moves as it would)
    if count.min() < 2:
        raise ValueError("pair_mutual_info: a label occurs once (scikit-learn drops such samples after its preparation; "
                         "the kernel does not imitate that)")
    if not _lib.lib.mlgnn_edge_mi_supported(n, n_nodes, n_pairs, k if -(1 << 31) <= k < 1 << 31 else 0, len(count),
                                            int(return_scores)):
        raise ValueError("pair_mutual_info: unsupported shape (%d samples, %d nodes, %d pairs, k = %d; 2 <= n <= %d, "
                         "k >= 1, below 4 GiB)" % (n, n_nodes, n_pairs, k, MAX_SAMPLES))
    if not torch.cuda.is_available():
        raise RuntimeError("mlgnn.edge_select.pair_mutual_info has no CPU path (the kernel is HIP only)")
    dev = x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device())
    mi = torch.zeros(n_pairs, dtype=torch.float64, device=dev)
    score = torch.zeros((n_pairs, n), dtype=torch.float64, device=dev) if return_scores else None
    counts = torch.zeros((n_pairs, n), dtype=torch.int32, device=dev) if return_counts else None
    if n_pairs:
        count_i = count[dense]
        k_i = np.minimum(k, count_i - 1)
        base = float(digamma(n) + np.mean(digamma(k_i)) - np.mean(digamma(count_i)))
        psi = np.zeros(n + 1, dtype=np.float64)
        psi[1:] = digamma(np.arange(1, n + 1))
        xt = x.detach().to(dev).to(torch.float64).t().contiguous()    # [n_nodes, n]: upcast and transpose on the device
        with torch.cuda.device(dev):
            _lib.call("mlgnn_edge_mi", xt, torch.from_numpy(p.astype(np.int32)).to(dev), torch.from_numpy(noise).to(dev),
                      torch.from_numpy(dense.astype(np.int32)).to(dev), torch.from_numpy(psi).to(dev), base, mi, score,
                      counts, n, n_nodes, n_pairs, k, len(count), _lib.stream())
    out = (mi.cpu().numpy(),)
    if return_scores:
        out += (score.cpu().numpy(),)
    if return_counts:
        out += (counts.cpu().numpy(),)
    return out if len(out) > 1 else out[0]


def sklearn_edge_select(values, y, edge_index, threshold=1.0, n_neighbors=3, random_state=None, mutual_classif=True,
                        pair_random_state=None):
    """The reference's loop (``valid_pca_mutual_info``), call for call: per edge ``PCA(n_components=1)`` on the two end
    columns and the mutual information of its score, the end columns' own cached per node.  As in the reference the
    regression path's pair call passes no ``random_state``: it takes ``pair_random_state``, whose default is the
    reference's.  (``n_neighbors`` is the reference's default of 3 there.)"""
    from sklearn.decomposition import PCA
    from sklearn.feature_selection import mutual_info_classif, mutual_info_regression
    x = _host(values).astype(np.float64, copy=False)
    y = _host(y).reshape(-1)
    ei = _host(edge_index).reshape(2, -1)
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
    if not (ENABLED and torch.cuda.is_available()):
        return False
    return edge_select_supported(n, n_nodes, n_edges + min(2 * n_edges, n_nodes), n_neighbors, counts_per_label,
                                 mutual_classif)


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
    ei = _host(edge_index)
    if ei.ndim != 2 or ei.shape[0] != 2:
        raise ValueError("edge_select: edge_index must be [2, E], got %s" % (ei.shape,))
    ei = ei.astype(np.int64)
    if getattr(values, "ndim", 0) != 2:
        raise ValueError("edge_select: values must be [n, n_nodes]")
    n, n_nodes, n_edges = int(values.shape[0]), int(values.shape[1]), int(ei.shape[1])
    if n_edges and (ei.min() < 0 or ei.max() >= n_nodes):
        raise ValueError("edge_select: node indices outside [0, %d)" % n_nodes)
    counts = _labels(y)[2]
    if use_kernel(n, n_nodes, n_edges, n_neighbors, counts, mutual_classif):
        EDGE_SELECT_STATS["hip"] += 1
        nodes = np.unique(ei)
        singles = np.stack([nodes, np.full_like(nodes, -1)], axis=1)
        mi = pair_mutual_info(values, y, np.concatenate([ei.T, singles], axis=0), n_neighbors, random_state)
        mi_pair, single = mi[:n_edges], mi[n_edges:]
        at = np.searchsorted(nodes, ei)
        keep = mi_pair > threshold * np.maximum(single[at[0]], single[at[1]])
        return keep, mi_pair, {int(v): float(m) for v, m in zip(nodes, single)}
    EDGE_SELECT_STATS["sklearn"] += 1
    return sklearn_edge_select(values, y, ei, threshold, n_neighbors, random_state, mutual_classif)
