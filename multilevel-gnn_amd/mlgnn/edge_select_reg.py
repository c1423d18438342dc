"""The ``--edge_select`` test of the fold preparation with ``mutual_classif`` false -- the reference's default -- on the
kernel of csrc/edge_select_cc.hip: the reference's ``valid_pca_mutual_info`` (``dataloader/multiloader.py:828-874``) keeps a
PPI edge iff ``mutual_info_regression`` between the label and the first principal component of its two end columns exceeds
``edge_select_threshold`` times the larger of the two end columns' own -- three scikit-learn calls per edge, three KD-trees
per call.  Here one launch computes a whole list of pairs and single columns, one workgroup each.

With a fixed ``random_state`` every ``mutual_info_regression`` call seeds a fresh generator and draws ``n`` normals for its
single feature, then ``n`` for the target: two noise vectors per seed, drawn on the host, are exactly what scikit-learn
adds.  The target is prepared on the host as :func:`mlgnn.mutual_info.prepare_regression` prepares it
(``scale(with_mean=False)`` plus its noise); ``base`` and the digamma table come from the host too.  The regression
estimator has no ``tree_path`` condition (scikit-learn's tree and its brute-force search compute the same Chebyshev
distances) and drops no sample.

The reference passes ``random_state`` to the end-node calls and none to the pair call (``:851``), so
:func:`edge_select_regression` takes two states.  Equal integer states: ONE launch over the ``E`` pairs and the ``U``
distinct end nodes.  Otherwise two launches, pairs and singles, each with its own draws; a launch whose state is ``None``
draws one unseeded noise pair where scikit-learn draws one per call.

:func:`edge_select_regression` runs the reference's own loop of scikit-learn calls on the host where the kernel does not
apply (switch off, no GPU, more than 2048 patients, ``k > 32``, ``k > n - 1``); that leg is the reference's arithmetic, not
a stand-in for a missing kernel.

Allocation: every device output is ``torch.zeros`` (as in :mod:`mlgnn.edge_select`); that the kernel writes every output
element whatever they held before is tested against the entry point directly (tests/test_edge_select_reg_gpu.py).  No
gradient, no ``autograd.Function``."""
import numbers
import os

import numpy as np
import torch

from . import _lib, _pairs
from .edge_select import sklearn_edge_select
from .mutual_info import MAX_NEIGHBORS_CC, MAX_SAMPLES

# MLGNN_EDGE_REG_FUSED=0: edge_select_regression always runs the loop of scikit-learn calls (same-box A/B runs).  The
# default follows the measurement of tools/bench_edge_select_reg.py (profiles/edge_select_reg.json, README "Edge selection,
# regression form"): end to end the kernel leg, in either of its forms, beats the scaled host leg by far more than that
# leg's spread at the gbm and kirc shapes.
DEFAULT_ENABLED = True
ENABLED = os.environ.get("MLGNN_EDGE_REG_FUSED", "1" if DEFAULT_ENABLED else "0") != "0"

# which leg edge_select_regression took.  A plain dict, not registered with _lib.stats, as for
# edge_select.EDGE_SELECT_STATS.
EDGE_SELECT_REG_STATS = {"hip": 0, "sklearn": 0}


def edge_select_regression_supported(n, n_nodes, n_pairs, n_neighbors, return_scores=False):
    """Whether the kernel takes the shape: ``2 <= n <= 2048``, ``1 <= n_neighbors <= min(n - 1, 32)``, the arrays below
    4 GiB.  The switch and the presence of a GPU are :func:`edge_select_regression`'s business."""
    k = int(n_neighbors)
    if not 1 <= k <= MAX_NEIGHBORS_CC:
        return False
    return bool(_lib.lib.mlgnn_edge_mi_cc_supported(int(n), int(n_nodes), int(n_pairs), k, int(return_scores)))


def prepare_target(y, random_state=None):
    """The host's share of one launch -> ``(noise_x [n], y_prepared [n])``: ``check_random_state(random_state)``, ``n``
    normals for the feature, then ``n`` for the target, and the target as ``mutual_info_regression`` prepares it."""
    from sklearn.preprocessing import scale
    from sklearn.utils import check_random_state
    y = np.ascontiguousarray(y, dtype=np.float64)
    rng = check_random_state(random_state)
    noise_x = rng.standard_normal(size=(y.size, 1))[:, 0]
    yp = scale(y, with_mean=False)
    yp += 1e-10 * np.maximum(1, np.mean(np.abs(yp))) * rng.standard_normal(size=y.size)
    return np.ascontiguousarray(noise_x), yp


def pair_mutual_info_regression(values, y, pairs, n_neighbors=3, random_state=None, return_scores=False,
                                return_counts=False):
    """``mutual_info_regression(PCA(n_components=1).fit_transform(values[:, [s, t]]), y, n_neighbors=...,
    random_state=...)`` for every row ``(s, t)`` of ``pairs [P, 2]``, and ``mutual_info_regression(values[:, [s]], y, ...)``
    for a row ``(s, -1)`` -> fp64 numpy ``[P]``.  ``values``: ``[n, n_nodes]`` fp32 or fp64 with any strides, on the host
    or the device (the upcast of fp32 is exact, so every form of the same values gives the same bits); ``y [n]``: any
    real column.  The noise is drawn on the host (:func:`prepare_target`), the same for every pair.  ``return_scores``:
    also the prepared columns ``[P, n]`` as handed to the estimator; ``return_counts``: also ``nx_i`` and ``ny_i`` as
    int32 ``[P, n]`` in sample order.  The caller checks :func:`edge_select_regression_supported` first."""
    k = int(n_neighbors)

    def prepare(target, n, n_nodes, n_pairs):
        from scipy.special import digamma
        noise_x, y_prepared = prepare_target(target, random_state)
        if not edge_select_regression_supported(n, n_nodes, n_pairs, k, return_scores):
            raise ValueError("pair_mutual_info_regression: unsupported shape (%d samples, %d nodes, %d pairs, k = %d; "
                             "2 <= n <= %d, 1 <= k <= min(n - 1, %d), below 4 GiB)"
                             % (n, n_nodes, n_pairs, k, MAX_SAMPLES, MAX_NEIGHBORS_CC))
        return (noise_x, y_prepared), digamma(n) + digamma(k), ()

    counts = torch.int32 if return_counts else None
    return _pairs.pair_op("mlgnn.edge_select_reg.pair_mutual_info_regression", "mlgnn_edge_mi_cc", values, y, np.float64,
                          pairs, prepare, (torch.float64 if return_scores else None, counts, counts), k)


def use_kernel(n, n_nodes, n_edges, n_neighbors):
    """:func:`edge_select_regression`'s dispatch rule: the kernel when ``MLGNN_EDGE_REG_FUSED`` is on, a GPU is present
    and :func:`edge_select_regression_supported` holds for the ``E`` pairs and at most ``min(2 E, n_nodes)`` singles."""
    return bool(ENABLED and torch.cuda.is_available()) and edge_select_regression_supported(
        n, n_nodes, _pairs.kernel_budget(n_edges, n_nodes), n_neighbors)


def _one_launch(random_state, pair_random_state):
    """Equal integer seeds: every call of the reference would draw the same noise, so one launch serves all rows."""
    return (isinstance(random_state, numbers.Integral) and isinstance(pair_random_state, numbers.Integral)
            and int(random_state) == int(pair_random_state))


def edge_select_regression(values, y, edge_index, threshold=1.0, n_neighbors=3, random_state=None, pair_random_state=None):
    """``valid_pca_mutual_info`` with ``mutual_classif`` false for every edge of ``edge_index [2, E]`` (node indices into
    the columns of ``values [n, n_nodes]``, the training patients' rows) -> ``(keep [E] bool, mi_pair [E] fp64, mi_node
    {node: value})``: edge ``e`` is kept iff ``mi_pair[e] > threshold * max(mi_node[src], mi_node[dst])``, decided on the
    host in fp64.  The end-node calls use ``random_state``, the pair calls ``pair_random_state`` (the reference passes
    none there, so ``None`` is its behaviour).  On the kernel: ONE launch over the ``E`` pairs and the ``U`` distinct
    end nodes when both states are the same integer, otherwise two launches (pairs, then singles); a launch whose state
    is ``None`` draws one unseeded noise pair where the reference draws one per scikit-learn call.  Otherwise the loop
    of scikit-learn calls runs.  ``EDGE_SELECT_REG_STATS`` counts the leg."""
    ei, n, n_nodes, n_edges = _pairs.check_edges(values, edge_index, "edge_select_regression")
    if not use_kernel(n, n_nodes, n_edges, n_neighbors):
        EDGE_SELECT_REG_STATS["sklearn"] += 1
        return sklearn_edge_select(values, y, ei, threshold, n_neighbors, random_state, mutual_classif=False,
                                   pair_random_state=pair_random_state)
    EDGE_SELECT_REG_STATS["hip"] += 1
    nodes, pairs = _pairs.launch_list(ei)
    if _one_launch(random_state, pair_random_state):
        mi = pair_mutual_info_regression(values, y, pairs, n_neighbors, random_state)
    else:
        mi = np.concatenate([pair_mutual_info_regression(values, y, pairs[:n_edges], n_neighbors, pair_random_state),
                             pair_mutual_info_regression(values, y, pairs[n_edges:], n_neighbors, random_state)])
    return _pairs.decide(mi, nodes, ei, threshold)
