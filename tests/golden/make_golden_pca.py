#!/usr/bin/env python3
"""Records ``pca_{0,1,2}.npz``: inputs of tests/_pca_ref.make_input and what scikit-learn's
``PCA(n_components=k_s, svd_solver='full')`` gives for every segment (``components_``, ``transform``,
``explained_variance_``, ``mean_``), zero-padded to ``k`` as mlgnn.pca.pathway_pca pads.  The scikit-learn version is
recorded too: the sign rule (``svd_flip(u_based_decision=False)``) is that of 1.5 and later.

  python tests/golden/make_golden_pca.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from _pca_ref import make_input, sklearn_pca  # noqa: E402

# (N, segment sizes, k, k_seg or None)
CASES = [
    (24, [6, 1, 0, 30, 3], 3, None),
    (50, [17, 50, 9, 2], 4, [2, 4, 0, 1]),
    (31, [40, 12, 5], 2, None),
]


def main():
    import sklearn
    for i, (n, sizes, k, k_seg) in enumerate(CASES):
        x, seg_ptr = make_input(n, sizes, seed=100 + i)
        comp, scores, var, mean = sklearn_pca(x, seg_ptr, k, k_seg=k_seg)
        path = os.path.join(HERE, "pca_%d.npz" % i)
        np.savez_compressed(path, x=x, seg_ptr=seg_ptr, k=np.int64(k),
                            k_seg=np.asarray(k_seg if k_seg is not None else [-1], dtype=np.int64),
                            components=comp, scores=scores, variance=var, mean=mean,
                            sklearn_version=np.array(sklearn.__version__))
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
