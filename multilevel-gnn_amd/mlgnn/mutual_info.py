"""The mutual-information gene mask on the kernel of csrc/mutual_info.hip: scikit-learn's ``mutual_info_classif`` for dense
continuous features (the estimator of Ross 2014, ``_compute_mi_cd``) with all features in one launch, one workgroup per
feature, instead of two KD-trees per column one column after another.

The host prepares the array with the calls scikit-learn makes -- ``check_X_y``, ``scale(with_mean=False)``, noise of
``1e-10 * max(1, mean|x|)`` drawn from ``check_random_state(random_state)`` -- so the kernel sees bit for bit the columns
``_compute_mi_cd`` sees and a fixed ``random_state`` gives the values it gives.  The preparation stays on the host on
purpose: it has to draw from numpy's generator.  The drop of samples whose label occurs once, the feature-independent
part of the estimate and the digamma table are host work too; the transpose to feature-major and everything per feature
run on the device.  fp64, no CPU path for the op; the models call scikit-learn where the op does not apply.

``mutual_info_regression`` (the estimator of Kraskov et al. 2004, ``_compute_mi_cc``: the k-th neighbour in the Chebyshev
metric of the (x, y) plane, then the counts inside that radius along x and along y) is the kernel of
csrc/mutual_info_cc.hip in the same way: :func:`prepare_regression` also scales the target and adds its noise from the
same generator after the features', and the kernel sees the arrays ``_compute_mi_cc`` sees.  scikit-learn's tree and its
brute-force search compute the same Chebyshev distances, so there is no :func:`tree_path` condition on this op."""
import os

import numpy as np
import torch

from . import _lib

# MLGNN_MI_FUSED=0: generate_mutual_mask of the models always calls scikit-learn (same-box A/B runs).  On by default: end
# to end the op beats the scikit-learn call by far more than that call's spread at the gbm, lgg and kirc shapes
# (profiles/mutual_info.json).
DEFAULT_ENABLED = True
ENABLED = os.environ.get("MLGNN_MI_FUSED", "1" if DEFAULT_ENABLED else "0") != "0"

# how often model_mutual_info took each path (development / tests: which path a mask was computed on)
class _RegressionCounters:
    """The report's suffix of the "mutual_info" line, rendered when the report is printed."""

    def __str__(self):
        return " regression %r (MLGNN_MI_REG_FUSED=%d)" % (MI_REG_STATS, REG_ENABLED)


MI_STATS = _lib.stats("mutual_info", _RegressionCounters(), hip=0, sklearn=0)

MAX_SAMPLES = 2048

# MLGNN_MI_REG_FUSED=1: generate_mutual_mask with mutual_classif false (the reference's default, mutual_info_regression:
# the Kraskov estimator) takes the kernel of csrc/mutual_info_cc.hip.  Off by default, and apart from ENABLED:
# tests/test_mutual_info_host.py::test_dispatch pins that the default routing sends mutual_classif=False to scikit-learn,
# and existing tests stay as they are; turning the default on is a later change that edits that test.
DEFAULT_REG_ENABLED = False
REG_ENABLED = os.environ.get("MLGNN_MI_REG_FUSED", "1" if DEFAULT_REG_ENABLED else "0") != "0"

# how often model_mutual_info took the regression kernel (its scikit-learn leg counts in MI_STATS["sklearn"], as before).
# A dict of its own, so that MI_STATS keeps its two keys; the MLGNN_PRINT_STATS report has one line per op and a fixed
# list of names (tests/test_binding_host.py), so these counters ride on the "mutual_info" line instead of a line of theirs.
MI_REG_STATS = {"hip": 0}

MAX_NEIGHBORS_CC = 32                                          # MLGNN_MI_CC_MAX_NEIGHBORS of include/mlgnn.h


def tree_path(k, counts_per_label):
    """Whether scikit-learn searches every label's neighbours with its tree, where its distances are ``|x - y|`` and the
    op returns its values: ``min(k, count - 1) < count // 2`` for every label that occurs more than once, the rule of
    ``NearestNeighbors(algorithm='auto')``.  Otherwise some label goes through the brute-force search, whose
    expanded-form distances the op does not imitate."""
    return all(min(int(k), int(c) - 1) < int(c) // 2 for c in counts_per_label if int(c) > 1)


def mutual_info_supported(n, n_features, k, counts_per_label):
    """Whether the op applies: ``n`` samples, of which those with a label occurring once are dropped (``counts_per_label``:
    how often each label occurs); at least 2 and at most 2048 must remain, ``k >= 1``, the array below 4 GiB."""
    kept = [int(c) for c in counts_per_label if int(c) > 1]
    if sum(int(c) for c in counts_per_label) != int(n) or not kept or int(k) < 1 or int(k) >= 1 << 31:
        return False
    return bool(_lib.lib.mlgnn_mutual_info_supported(sum(kept), int(n_features), int(k), len(kept)))


def digamma_table(n):
    """``psi[c] = digamma(c)`` for ``c = 1 .. n`` as fp64 ``[n + 1]`` (``psi[0] = 0`` is never read): the table every
    mutual-information kernel looks its neighbour counts up in."""
    from scipy.special import digamma
    psi = np.zeros(n + 1, dtype=np.float64)
    psi[1:] = digamma(np.arange(1, n + 1))
    return psi


def _scale_and_noise(X, rng):
    """The lines of scikit-learn's ``_estimate_mi`` for dense continuous features: ``scale(with_mean=False)``, then noise
    of ``1e-10 * max(1, mean|x|)`` per column, the first draw from ``rng`` -> a new fp64 array."""
    from sklearn.preprocessing import scale
    n_samples, n_features = X.shape
    continuous_mask = np.ones(n_features, dtype=bool)          # dense input: every feature is continuous
    X = X.astype(np.float64, copy=True)
    X[:, continuous_mask] = scale(X[:, continuous_mask], with_mean=False, copy=False)
    means = np.maximum(1, np.mean(np.abs(X[:, continuous_mask]), axis=0))
    X[:, continuous_mask] += 1e-10 * means * rng.standard_normal(size=(n_samples, np.sum(continuous_mask)))
    return X


def prepare(x, y, random_state=None):
    """``mutual_info_classif``'s preparation of dense continuous features, call for call -> ``(X [n, F] fp64, y [n])``."""
    from sklearn.utils import check_random_state
    from sklearn.utils.validation import check_X_y
    X, y = check_X_y(x, y, accept_sparse="csc", y_numeric=False)
    return _scale_and_noise(X, check_random_state(random_state)), y


def mutual_info_cd(prepared, y, n_neighbors=3, return_counts=False):
    """The estimator on an already prepared fp64 array ``[n, F]`` (tests; :func:`mutual_info_classif` is this after
    :func:`prepare`).  ``return_counts``: also ``m_i`` as int32 ``[F, n_kept]`` in the order of the kept samples, and the
    boolean mask ``[n]`` of the kept samples."""
    from scipy.special import digamma
    X = np.ascontiguousarray(prepared, dtype=np.float64)
    y = np.asarray(y)
    if X.ndim != 2 or y.shape != (X.shape[0],):
        raise ValueError("mutual_info_cd: prepared %s, y %s" % (X.shape, y.shape))
    n_features = X.shape[1]
    k = int(n_neighbors)
    _, dense, count = np.unique(y, return_inverse=True, return_counts=True)
    keep = count[dense] > 1                                    # scikit-learn: "ignore points with unique labels"
    n = int(keep.sum())
    if n == 0 or n_features == 0:
        mi = np.zeros(n_features, dtype=np.float64)
        return (mi, np.zeros((n_features, 0), dtype=np.int32), keep) if return_counts else mi
    if not torch.cuda.is_available():
        raise RuntimeError("mlgnn.mutual_info has no CPU path (the kernel is HIP only)")
    _, d, c = np.unique(y[keep], return_inverse=True, return_counts=True)
    if not _lib.lib.mlgnn_mutual_info_supported(n, n_features, k, len(c)):
        raise ValueError("mutual_info_cd: unsupported shape (%d samples after the drop, %d features, k = %d; 2 <= n <= %d, "
                         "k >= 1, below 4 GiB)" % (n, n_features, k, MAX_SAMPLES))
    count_i = c[d]
    k_i = np.minimum(k, count_i - 1)
    base = float(digamma(n) + np.mean(digamma(k_i)) - np.mean(digamma(count_i)))
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = X if n == X.shape[0] else X[keep]
    xt = torch.from_numpy(rows).to(dev).t().contiguous()       # [F, n]: the transpose runs on the device
    labels = torch.from_numpy(d.astype(np.int32)).to(dev)
    psi_d = torch.from_numpy(digamma_table(n)).to(dev)
    mi = torch.empty(n_features, dtype=torch.float64, device=dev)
    counts = torch.empty((n_features, n), dtype=torch.int32, device=dev) if return_counts else None
    _lib.call("mlgnn_mutual_info_cd", xt, labels, psi_d, base, mi, counts, n, n_features, k, len(c), _lib.stream())
    out = mi.cpu().numpy()
    return (out, counts.cpu().numpy(), keep) if return_counts else out


def mutual_info_classif(x, y, n_neighbors=3, random_state=None, return_counts=False):
    """``sklearn.feature_selection.mutual_info_classif(x, y, n_neighbors=..., random_state=...)`` for dense continuous
    features -> fp64 numpy ``[F]`` (with ``return_counts`` also the ``m_i`` and the kept-sample mask of
    :func:`mutual_info_cd`).  The values are scikit-learn's where :func:`tree_path` holds; the caller checks that and
    :func:`mutual_info_supported` first."""
    X, y = prepare(x, y, random_state)
    return mutual_info_cd(X, y, n_neighbors, return_counts)


def mutual_info_regression_supported(n, n_features, k):
    """Whether the regression op applies: ``2 <= n <= 2048``, ``1 <= k <= min(n - 1, 32)``, the array below 4 GiB."""
    if not -(1 << 31) <= int(k) < 1 << 31:
        return False
    return bool(_lib.lib.mlgnn_mutual_info_cc_supported(int(n), int(n_features), int(k)))


def prepare_regression(x, y, random_state=None):
    """``mutual_info_regression``'s preparation of dense continuous features and a continuous target, call for call (the
    lines of ``_estimate_mi`` with ``discrete_target=False``; every draw from the one generator, ``X`` first) ->
    ``(X [n, F] fp64, y [n] fp64)``."""
    from sklearn.preprocessing import scale
    from sklearn.utils import check_random_state
    from sklearn.utils.validation import check_X_y
    X, y = check_X_y(x, y, accept_sparse="csc", y_numeric=True)
    rng = check_random_state(random_state)
    X = _scale_and_noise(X, rng)
    y = scale(y, with_mean=False)
    y += 1e-10 * np.maximum(1, np.mean(np.abs(y))) * rng.standard_normal(size=X.shape[0])
    return X, y


def mutual_info_cc(prepared, y_prepared, n_neighbors=3, return_counts=False):
    """The Kraskov estimator on already prepared fp64 arrays ``[n, F]`` and ``[n]`` (tests;
    :func:`mutual_info_regression` is this after :func:`prepare_regression`).  ``return_counts``: also ``nx_i`` and
    ``ny_i`` as int32 ``[F, n]`` in the input's sample order."""
    from scipy.special import digamma
    X = np.ascontiguousarray(prepared, dtype=np.float64)
    y = np.ascontiguousarray(y_prepared, dtype=np.float64)
    if X.ndim != 2 or y.shape != (X.shape[0],):
        raise ValueError("mutual_info_cc: prepared %s, y %s" % (X.shape, y.shape))
    n, n_features = X.shape
    k = int(n_neighbors)
    if not torch.cuda.is_available():
        raise RuntimeError("mlgnn.mutual_info has no CPU path (the kernel is HIP only)")
    if not mutual_info_regression_supported(n, n_features, k):
        raise ValueError("mutual_info_cc: unsupported shape (%d samples, %d features, k = %d; 2 <= n <= %d, "
                         "1 <= k <= min(n - 1, %d), below 4 GiB)" % (n, n_features, k, MAX_SAMPLES, MAX_NEIGHBORS_CC))
    if n_features == 0:
        mi = np.zeros(0, dtype=np.float64)
        return (mi, np.zeros((0, n), dtype=np.int32), np.zeros((0, n), dtype=np.int32)) if return_counts else mi
    base = float(digamma(n) + digamma(k))
    dev = torch.device("cuda", torch.cuda.current_device())
    xt = torch.from_numpy(X).to(dev).t().contiguous()          # [F, n]: the transpose runs on the device
    y_d = torch.from_numpy(y).to(dev)
    psi_d = torch.from_numpy(digamma_table(n)).to(dev)
    mi = torch.empty(n_features, dtype=torch.float64, device=dev)
    nx = torch.empty((n_features, n), dtype=torch.int32, device=dev) if return_counts else None
    ny = torch.empty((n_features, n), dtype=torch.int32, device=dev) if return_counts else None
    _lib.call("mlgnn_mutual_info_cc", xt, y_d, psi_d, base, mi, nx, ny, n, n_features, k, _lib.stream())
    out = mi.cpu().numpy()
    return (out, nx.cpu().numpy(), ny.cpu().numpy()) if return_counts else out


def mutual_info_regression(x, y, n_neighbors=3, random_state=None, return_counts=False):
    """``sklearn.feature_selection.mutual_info_regression(x, y, n_neighbors=..., random_state=...)`` for dense
    continuous features -> fp64 numpy ``[F]`` (with ``return_counts`` also the ``nx_i`` and ``ny_i`` of
    :func:`mutual_info_cc`).  The caller checks :func:`mutual_info_regression_supported` first."""
    X, y = prepare_regression(x, y, random_state)
    return mutual_info_cc(X, y, n_neighbors, return_counts)


def label_counts(y):
    """How often each label of ``y`` occurs (the ``counts_per_label`` of :func:`tree_path`, :func:`mutual_info_supported`)."""
    y = y.detach().cpu().numpy() if torch.is_tensor(y) else np.asarray(y)
    return np.unique(y, return_counts=True)[1]


def model_mutual_info(x, y, n_neighbors, random_state, mutual_classif):
    """The mutual information ``generate_mutual_mask`` of the models thresholds: the kernel when ``mutual_classif`` is
    true, the switch is on, a GPU is present, the shape is supported and :func:`tree_path` holds; with ``mutual_classif``
    false the regression kernel when its switch (``REG_ENABLED``, off by default) is on, a GPU is present and the shape
    is supported; otherwise the scikit-learn call (small classes, CPU-only hosts, more than 2048 samples, ``k`` above
    the regression kernel's cap)."""
    plain = getattr(x, "ndim", 0) == 2 and getattr(y, "ndim", 0) == 1
    if mutual_classif and ENABLED and torch.cuda.is_available() and plain:
        counts = label_counts(y)
        if mutual_info_supported(x.shape[0], x.shape[1], n_neighbors, counts) and tree_path(n_neighbors, counts):
            MI_STATS["hip"] += 1
            return mutual_info_classif(x, y, n_neighbors=n_neighbors, random_state=random_state)
    if not mutual_classif and REG_ENABLED and torch.cuda.is_available() and plain \
            and mutual_info_regression_supported(x.shape[0], x.shape[1], n_neighbors):
        MI_REG_STATS["hip"] += 1
        return mutual_info_regression(x, y, n_neighbors=n_neighbors, random_state=random_state)
    import sklearn.feature_selection as fs
    fn = fs.mutual_info_classif if mutual_classif else fs.mutual_info_regression
    MI_STATS["sklearn"] += 1
    return fn(x, y, n_neighbors=n_neighbors, random_state=random_state)
