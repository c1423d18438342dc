#!/usr/bin/env python3
"""Generate ``tests/golden/kraskov_0.npz`` from the reference's OWN ``utils/knnie.py::kraskov_mi``.

Run where the reference tree is present:  ``MLGNN_REFERENCE=<tree> python tests/golden/make_golden_kraskov.py``.  The
reference never travels;
the ``.npz`` written next to this script does.  Nothing in the test-suite imports this file.

``utils/knnie.py`` imports ``cvxopt`` (and ``matplotlib``) at module level and uses neither in ``kraskov_mi``; where one
is not installed an empty *import-only* module is registered under its name.  Everything ``kraskov_mi`` calls -- scipy's
``cKDTree`` and ``digamma`` -- is the installed library.

The fixture: a ``[60, 8]`` fp64 value matrix (six continuous columns carrying the label with different strengths, one
quantised to sixteenths, one of scale 1e3), a 0/1 label as a float column, 28 pairs and 8 singles (the call forms of
``valid_pca_mutual_info``, multiloader.py:838-839, 853-854, 863-864), and ``kraskov_mi``'s result for each at its default
``k = 5``."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("MLGNN_REFERENCE")                 # the reference tree, as for make_golden.py
N, N_NODES, K, SEED = 60, 8, 5, 20240


def _reference_knnie():
    if not REF:
        raise SystemExit("set MLGNN_REFERENCE to the reference tree")
    for name, members in (("cvxopt", ("matrix", "solvers")), ("matplotlib", ()), ("matplotlib.pyplot", ())):
        try:
            __import__(name)
        except ImportError:
            mod = types.ModuleType(name)
            for member in members:
                setattr(mod, member, None)
            sys.modules[name] = mod
    spec = importlib.util.spec_from_file_location("reference_knnie", os.path.join(REF, "utils", "knnie.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def main():
    knnie = _reference_knnie()
    rng = np.random.RandomState(SEED)
    y = (rng.rand(N) < 0.45).astype(np.float64)
    values = rng.standard_normal((N, N_NODES)) + y[:, None] * np.linspace(0.0, 2.1, N_NODES)[None, :]
    values[:, 6] = np.round(16.0 * values[:, 6]) / 16.0
    values[:, 7] *= 1e3
    pairs = [(s, t) for s in range(N_NODES) for t in range(s + 1, N_NODES)] + [(s, -1) for s in range(N_NODES)]
    pairs = np.array(pairs, dtype=np.int64)
    mi = np.array([knnie.kraskov_mi(values[:, [s, t] if t >= 0 else [s]], y[:, None], k=K) for s, t in pairs.tolist()])
    assert np.isfinite(mi).all()
    out = os.path.join(HERE, "kraskov_0.npz")
    np.savez(out, values=values, y=y, pairs=pairs, k=np.int64(K), mi=mi)
    print("wrote %s: %d pairs, mi in [%.4f, %.4f]" % (out, len(pairs), mi.min(), mi.max()))


if __name__ == "__main__":
    main()
