#!/usr/bin/env python3
"""Generate ``tests/golden/ksg_mi_{0,1,2}.npz`` from scikit-learn's own ``mutual_info_regression`` (the Kraskov
estimator, ``_compute_mi_cc``).

Run in the authoring container only:  ``python tests/golden/make_golden_ksg_mi.py``.  Nothing in the test-suite imports
this file.  (Not named ``mutual_info_*``: the tests of the classif op glob that prefix.)  One fixture each of a
two-valued label target on noisy values, the same on values rounded to halves, and a continuous target.  Recorded: the
raw ``x`` (fp32), ``y`` (fp64), ``k``, ``seed`` (the ``random_state``), ``prepared`` and ``y_prepared`` -- the fp64
columns and target ``_compute_mi`` was handed, captured inside the call -- the returned ``mi``, and the versions of
scikit-learn, numpy and scipy that computed it."""
import os
import sys

import numpy as np
import scipy
import sklearn
import sklearn.feature_selection._mutual_info as skmi

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from _mi_ref import make_input  # noqa: E402

# (label counts, F, k, halves, continuous target)
CASES = [((63, 34), 24, 7, False, False), ((60, 40), 24, 15, True, False), ((24, 16), 20, 3, False, True)]


def record(x, y, k, seed):
    cols, targets = [], []
    inner = skmi._compute_mi

    def spy(c, d, *rest):
        cols.append(np.array(c, dtype=np.float64, copy=True))
        targets.append(np.array(d, dtype=np.float64, copy=True))
        return inner(c, d, *rest)

    skmi._compute_mi = spy
    try:
        mi = skmi.mutual_info_regression(x, y, n_neighbors=k, random_state=seed)
    finally:
        skmi._compute_mi = inner
    assert all(np.array_equal(t, targets[0]) for t in targets)
    return np.stack(cols, axis=1), targets[0], mi


def main():
    for ci, (counts, F, k, halves, cont) in enumerate(CASES):
        seed = 2000 + ci
        x, labels = make_input(counts, F, seed, halves)
        y = labels.astype(np.float64)
        if cont:
            y = y + np.random.RandomState(seed + 1).standard_normal(len(y))
        prepared, y_prepared, mi = record(x, y, k, seed)
        assert prepared.shape == x.shape and y_prepared.shape == y.shape and mi.shape == (F,)
        path = os.path.join(HERE, "ksg_mi_%d.npz" % ci)
        np.savez_compressed(path, x=x, y=y, k=np.array(k), seed=np.array(seed), prepared=prepared, y_prepared=y_prepared,
                            mi=mi, sklearn=np.array(sklearn.__version__), numpy=np.array(np.__version__),
                            scipy=np.array(scipy.__version__))
        print(ci, counts, F, k, "halves" if halves else "", "cont" if cont else "label", "mi max %.4f" % mi.max(),
              os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
