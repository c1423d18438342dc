#!/usr/bin/env python3
"""Generate ``tests/golden/mutual_info_{0..}.npz`` from scikit-learn's own ``mutual_info_classif``.

Run in the authoring container only:  ``python tests/golden/make_golden_mi.py``.  Nothing in the test-suite imports this
file.  Every fixture is an input on which scikit-learn searches each label's neighbours with its tree
(``min(k, count - 1) < count // 2`` for every label).  Recorded: the raw ``x`` (fp32), ``y``, ``k``, ``seed`` (the
``random_state``), ``prepared`` -- the fp64 array whose columns ``_compute_mi`` was handed, captured inside the call --
the returned ``mi``, and the versions of scikit-learn, numpy and scipy that computed it."""
import os
import sys

import numpy as np
import scipy
import sklearn
import sklearn.feature_selection._mutual_info as skmi

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from _mi_ref import make_input  # noqa: E402

# (label counts, F, k, halves)
CASES = [((24, 16), 50, 3, False), ((63, 34), 64, 7, False), ((217, 83), 24, 15, False), ((86, 86, 85), 24, 15, False),
         ((63, 34), 32, 7, True), ((86, 86, 85), 16, 15, True), ((30, 1, 25), 20, 3, False)]


def record(x, y, k, seed):
    cols = []
    inner = skmi._compute_mi

    def spy(c, d, *rest):
        cols.append(np.array(c, dtype=np.float64, copy=True))
        return inner(c, d, *rest)

    skmi._compute_mi = spy
    try:
        mi = skmi.mutual_info_classif(x, y, n_neighbors=k, random_state=seed)
    finally:
        skmi._compute_mi = inner
    return np.stack(cols, axis=1), mi


def main():
    for ci, (counts, F, k, halves) in enumerate(CASES):
        assert all(min(k, c - 1) < c // 2 for c in counts if c > 1), counts
        seed = 1000 + ci
        x, y = make_input(counts, F, seed, halves)
        prepared, mi = record(x, y, k, seed)
        assert prepared.shape == x.shape and mi.shape == (F,)
        np.savez_compressed(os.path.join(HERE, "mutual_info_%d.npz" % ci), x=x, y=y, k=np.array(k), seed=np.array(seed),
                            prepared=prepared, mi=mi, sklearn=np.array(sklearn.__version__),
                            numpy=np.array(np.__version__), scipy=np.array(scipy.__version__))
        print(ci, counts, F, k, "halves" if halves else "", "mi max %.4f" % mi.max())


if __name__ == "__main__":
    main()
