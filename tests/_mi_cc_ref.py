"""numpy restatement of the Kraskov mutual-information estimator of csrc/mutual_info_cc.hip (include/mlgnn.h), an O(N^2)
loop per column on already prepared fp64 arrays:

    d_ij = max(fl|x_j - x_i|, fl|y_j - y_i|)
    r_i  = the k-th smallest d_ij over j != i
    rr_i = nextafter(r_i, 0)
    nx_i = #{ j != i : fl|x_j - x_i| <= rr_i },  ny_i = #{ j != i : fl|y_j - y_i| <= rr_i }
    mi   = max(0, psi(N) + psi(k) - mean_i psi(nx_i + 1) - mean_i psi(ny_i + 1))

The last line is written with the four terms in scikit-learn's order (``_compute_mi_cc``), so that the values agree with
it to the last bit, on its tree path and on its brute-force path alike (Chebyshev distances have no expanded form).  Also
the inputs the tests of the op share: :func:`make_target`, :func:`prepared_case` and the case table."""
import numpy as np
from scipy.special import digamma

from _mi_ref import make_input


def mi_cc_ref(prepared, y_prepared, k):
    """prepared [n, F] fp64, y_prepared [n] fp64 -> (mi [F] fp64, nx [F, n] int64, ny [F, n] int64), sample order."""
    X = np.asarray(prepared, dtype=np.float64)
    y = np.asarray(y_prepared, dtype=np.float64)
    n, F = X.shape
    off = ~np.eye(n, dtype=bool)
    dy = np.abs(y[None, :] - y[:, None])                               # dy[i, j] = fl|y_j - y_i|
    mi = np.empty(F)
    nx_all = np.empty((F, n), dtype=np.int64)
    ny_all = np.empty((F, n), dtype=np.int64)
    for f in range(F):
        c = X[:, f]
        dx = np.abs(c[None, :] - c[:, None])
        d = np.maximum(dx, dy)[off].reshape(n, n - 1)                  # j != i
        r = np.partition(d, k - 1, axis=1)[:, k - 1]
        rr = np.nextafter(r, 0)[:, None]
        nx = ((dx <= rr) & off).sum(axis=1)
        ny = ((dy <= rr) & off).sum(axis=1)
        nx_all[f], ny_all[f] = nx, ny
        v = digamma(n) + digamma(k) - np.mean(digamma(nx + 1.0)) - np.mean(digamma(ny + 1.0))
        mi[f] = max(0, v)
    return mi, nx_all, ny_all


def make_target(labels, kind, seed):
    """The raw target of a case: the label as float (what train.py passes), or ``label + N(0, 1)`` ("cont")."""
    y = np.asarray(labels, dtype=np.float64)
    if kind == "cont":
        y = y + np.random.RandomState(seed + 1000).standard_normal(len(y))
    return y


# name -> (label counts, F, k, how the prepared arrays are made, target)
CASES = {
    "n2_k1": ((1, 1), 4, 1, "noise", "label"),
    "n3_k2": ((2, 1), 4, 2, "noise", "label"),
    "n40": ((24, 16), 50, 3, "noise", "label"),
    "n97": ((63, 34), 24, 7, "noise", "label"),
    "n97_cont": ((63, 34), 24, 7, "noise", "cont"),
    "n97_halves": ((63, 34), 24, 7, "halves", "label"),
    "n300": ((217, 83), 12, 15, "noise", "label"),
    "n300_halves": ((217, 83), 12, 15, "halves", "label"),
    "n300_cont_halves": ((217, 83), 12, 15, "halves", "cont"),
    "duplicates_without_noise_k3": ((40, 30, 27), 16, 3, "exact", "label"),
    "brute_path_n40_k20": ((24, 16), 12, 20, "noise", "label"),
    "whole_column_n17_k16": ((10, 7), 8, 16, "noise", "cont"),
    "k_at_the_cap_n33_k32": ((20, 13), 8, 32, "noise", "label"),
    "n2048": ((1024, 1024), 4, 15, "noise", "label"),
    "n2047_cont_halves": ((1030, 1017), 4, 7, "halves", "cont"),
    "more_workgroups_than_cus": ((32, 32), 3000, 3, "noise", "label"),
}
SMALL = [name for name, case in CASES.items() if sum(case[0]) <= 300]     # the cases the host test runs scikit-learn on

_PREPARED = {}


def prepared_case(name, seed=21):
    """``(prepared X [n, F], prepared y [n], k)`` of a case; computed once and shared (callers do not write to them).
    "exact": no scaling and no noise, so exact duplicates stay in x and in y (the r_i = 0 branch)."""
    if name not in _PREPARED:
        from mlgnn.mutual_info import prepare_regression
        counts, F, k, how, target = CASES[name]
        x, labels = make_input(counts, F, seed, halves=(how != "noise"))
        y = make_target(labels, target, seed)
        if how == "exact":
            X, yp = x.astype(np.float64), y.copy()
        else:
            X, yp = prepare_regression(x, y, seed + 1)
        _PREPARED[name] = (X, yp, k)
    return _PREPARED[name]


_REFERENCE = {}


def reference_case(name):
    """:func:`mi_cc_ref` of a case, computed once."""
    if name not in _REFERENCE:
        X, yp, k = prepared_case(name)
        _REFERENCE[name] = mi_cc_ref(X, yp, k)
    return _REFERENCE[name]
