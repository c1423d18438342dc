#!/usr/bin/env python3
"""The ``--edge_select`` test of the fold preparation (``valid_pca_mutual_info`` per PPI edge) at the ``(n, E)`` of the gbm
and kirc training folds on :class:`mlgnn.data.SyntheticTCGA`,

  (n, E) = (200, 60000)   gbm
           (300, 60000)   kirc

with the label planted in every node (the cohort's own values are independent uniform draws).  Times
``mlgnn.edge_select.edge_select`` on the kernel of csrc/edge_select.hip against the same call with the switch off (the
reference's loop of scikit-learn calls), same input and ``random_state``, with the protocol of tools/bench_mutual_info.py:
wall clock with a device synchronise, the two legs alternating over three repeats so the scikit-learn leg's spread is on
record, the kernel alone by device events, one untimed call first.  The scikit-learn leg runs on a fixed subsample of
``--sklearn_edges`` edges (three scikit-learn calls per edge: the whole fold takes minutes); its time per edge is reported
and scaled to ``E`` at one third (the whole fold caches the end nodes' values, so only the pair call is certain per edge:
a lower bound of the loop's time), and the JSON says so.  Both legs' decisions are compared on the subsample.

``ships_enabled`` is the rule for the default of ``MLGNN_EDGE_SELECT_FUSED``: the kernel leg on ALL edges beats the scaled
scikit-learn leg by more than that leg's scaled spread at both shapes.  Writes profiles/edge_select.json.  Development
tool; every shape runs in a fresh child process under ``--step_limit`` (``drive`` of tools/_bench.py)."""
import importlib
import os

import numpy as np

import _edge_bench as frame
from _bench import beats, leg_summary, switched, wall
from _edge_bench import make_fold

ES = importlib.import_module("mlgnn.edge_select")
SEED, K = 12345, 3


def kernel_ms(x, y, ei, warmup, iters):
    """The launch of mlgnn_edge_mi alone (E pairs + U singles), operands resident on the device."""
    from scipy.special import digamma
    from sklearn.utils import check_random_state
    _, d, c = np.unique(y, return_inverse=True, return_counts=True)
    base = digamma(len(y)) + np.mean(digamma(np.minimum(K, c[d] - 1))) - np.mean(digamma(c[d]))
    vectors = (check_random_state(SEED).standard_normal(len(y)), d.astype(np.int32))
    return frame.kernel_ms("mlgnn_edge_mi", x, ei, vectors, base, K, 2, (len(c),), warmup, iters)


def bench_shape(name, n, n_edges, sub, warmup, iters, repeats):
    x, y, ei = make_fold(n, n_edges)
    E = ei.shape[1]
    pick = np.random.RandomState(3).choice(E, size=min(sub, E), replace=False)
    entry = {"shape": name, "n": n, "E": E, "n_nodes": int(x.shape[1]), "k": K, "sklearn_edges": int(len(pick)),
             "sklearn_leg": "a fixed subsample of the edges, where nearly every end node is new to the cache (three "
                            "scikit-learn calls per edge); scaled to E at ONE THIRD of its per-edge time, the pair call "
                            "alone, which every edge of the whole fold needs: a lower bound of the loop's time",
             "hip_end_to_end_ms": [], "sklearn_subsample_ms": [], "kernel_ms": []}
    got = want = None
    for _ in range(repeats):                                                  # the legs alternate
        ms, got = wall(lambda: ES.edge_select(x, y, ei, 1.0, K, SEED))
        entry["hip_end_to_end_ms"].append(ms)
        with switched(ES, "ENABLED", False):
            ms, want = wall(lambda: ES.edge_select(x, y, ei[:, pick], 1.0, K, SEED))
        entry["sklearn_subsample_ms"].append(ms)
        ms, launched = kernel_ms(x, y, ei, warmup, iters)
        entry["kernel_ms"].append(ms)
        entry["pairs_per_launch"] = launched
    top = np.array([max(want[2][int(s)], want[2][int(t)]) for s, t in ei[:, pick].T])
    clear = np.abs(want[1] - top) > 1e-9
    entry["max_abs_diff_to_sklearn"] = float(np.abs(got[1][pick] - want[1]).max())
    entry["edges_inside_the_1e-9_margin"] = int((~clear).sum())
    entry["decisions_equal_outside_the_margin"] = bool(np.array_equal(got[0][pick][clear], want[0][clear]))
    entry["kept_by_the_kernel_leg"] = int(got[0].sum())
    scale = E / len(pick) / 3.0
    hip, ref = entry["hip_end_to_end_ms"], [ms * scale for ms in entry["sklearn_subsample_ms"]]
    h, r = leg_summary(hip), leg_summary(ref)
    entry["summary"] = {"hip_end_to_end_mean_ms": h["mean"], "hip_spread_ms": h["spread"],
                        "sklearn_per_edge_ms": leg_summary(entry["sklearn_subsample_ms"])["mean"] / len(pick),
                        "sklearn_scaled_mean_ms": r["mean"], "sklearn_scaled_spread_ms": r["spread"],
                        "kernel_mean_ms": leg_summary(entry["kernel_ms"])["mean"],
                        "speedup_over_sklearn": sum(ref) / sum(hip),
                        "beats_sklearn_by_more_than_its_spread": beats(hip, ref)}
    return entry


def main():
    a = frame.arguments("sklearn_edges", "edge_select.json")
    if a.child:
        import scipy
        import sklearn
        with switched(ES, "ENABLED", True):
            return frame.run_shape(os.path.basename(__file__), a.child,
                                   lambda n, n_edges: ES.edge_select(*make_fold(n, n_edges), 1.0, K, SEED),
                                   lambda *shape: bench_shape(*shape, a.sklearn_edges, a.warmup, a.iters, a.repeats),
                                   (sklearn, np, scipy))
    result = {"workload": "valid_pca_mutual_info for every PPI edge of a fold (PCA(n_components=1) of the two end columns, "
                          "mutual_info_classif of its score and of each end column, fp64): edge_select on the kernel of "
                          "csrc/edge_select.hip (MLGNN_EDGE_SELECT_FUSED=1) against the loop of scikit-learn calls, same "
                          "input and random_state",
              "timing": "one child process per shape under a limit of %g s; in it wall clock around each call with a "
                        "device synchronise, the two legs alternating over %d repeats; the kernel alone by device events, "
                        "mean of %d launches after %d; one untimed call of the kernel leg first"
                        % (a.step_limit, a.repeats, a.iters, a.warmup)}
    frame.drive(__file__, a, "sklearn_edges", result, "beats_sklearn_by_more_than_its_spread")


if __name__ == "__main__":
    main()
