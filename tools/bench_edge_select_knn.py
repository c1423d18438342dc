#!/usr/bin/env python3
"""The ``--knn_mutual_info`` form of the fold preparation's edge test (``kraskov_mi`` per PPI edge and end node) at the
``(n, E)`` of the gbm and kirc training folds on :class:`mlgnn.data.SyntheticTCGA`,

  (n, E) = (200, 60000)   gbm
           (300, 60000)   kirc

with the label planted in every node, as in tools/bench_edge_select.py, whose protocol this follows: wall clock with a
device synchronise, the two legs alternating over three repeats so the host leg's spread is on record, the kernel alone by
device events, one untimed call first.  Times ``mlgnn.kraskov.edge_select_knn`` on the kernel of csrc/kraskov_mi.hip
against the same call with the switch off (three ``scipy.spatial.cKDTree`` per call, the reference's arithmetic).  The
host leg runs on a fixed subsample of ``--host_edges`` edges (the whole fold takes minutes); its time is scaled to ``E`` at
the PAIR call alone -- the subsample's end-node calls are timed apart and left out, since the whole fold computes each end
node once: a lower bound of the loop's time -- and the JSON says so.  Both legs' values and decisions are compared on the
subsample.

``ships_enabled`` is the rule for the default of ``MLGNN_EDGE_KNN_FUSED``: the kernel leg on ALL edges beats the scaled
host leg by more than that leg's scaled spread at both shapes.  Writes profiles/edge_select_knn.json.  Development tool;
every shape runs in a fresh child process under ``--step_limit`` (``drive`` of tools/_bench.py)."""
import importlib
import os

import numpy as np

import _edge_bench as frame
from _bench import beats, leg_summary, switched, wall

KN = importlib.import_module("mlgnn.kraskov")
K = 5


def make_fold(n, n_edges):
    return frame.make_fold(n, n_edges, np.float64)


def kernel_ms(x, y, ei, warmup, iters):
    """The launch of mlgnn_kraskov_mi alone (E pairs + U singles), operands resident on the device."""
    from scipy.special import digamma
    return frame.kernel_ms("mlgnn_kraskov_mi", x, ei, (y,), digamma(K) + digamma(len(y)), K, 3, (), warmup, iters)


def bench_shape(name, n, n_edges, sub, warmup, iters, repeats):
    x, y, ei = make_fold(n, n_edges)
    E = ei.shape[1]
    pick = np.random.RandomState(3).choice(E, size=min(sub, E), replace=False)
    x_host = x.numpy()
    singles, rows = frame.launch_list(ei[:, pick])
    single_pairs = rows[len(pick):]
    entry = {"shape": name, "n": n, "E": E, "n_nodes": int(x.shape[1]), "k": K, "host_edges": int(len(pick)),
             "host_leg": "kraskov_mi_host on a fixed subsample of the edges; scaled to E at the PAIR calls alone (the "
                         "subsample's end-node calls are timed apart and left out: the whole fold computes each end node "
                         "once): a lower bound of the loop's time",
             "hip_end_to_end_ms": [], "host_pair_calls_ms": [], "host_node_calls_ms": [], "kernel_ms": []}
    got = pair = node = None
    for _ in range(repeats):                                                  # the legs alternate
        ms, got = wall(lambda: KN.edge_select_knn(x, y, ei, 1.0, K))
        entry["hip_end_to_end_ms"].append(ms)
        ms, pair = wall(lambda: KN.kraskov_mi_host(x_host, y, ei[:, pick].T, K))
        entry["host_pair_calls_ms"].append(ms)
        ms, node = wall(lambda: KN.kraskov_mi_host(x_host, y, single_pairs, K))
        entry["host_node_calls_ms"].append(ms)
        ms, launched = kernel_ms(x, y, ei, warmup, iters)
        entry["kernel_ms"].append(ms)
        entry["pairs_per_launch"] = launched
    at = np.searchsorted(singles, ei[:, pick])
    top = np.maximum(node[at[0]], node[at[1]])
    clear = np.abs(pair - top) > 1e-9
    entry["max_abs_diff_to_host"] = float(max(np.abs(got[1][pick] - pair).max(),
                                              max(abs(got[2][int(v)] - m) for v, m in zip(singles, node))))
    entry["edges_inside_the_1e-9_margin"] = int((~clear).sum())
    entry["decisions_equal_outside_the_margin"] = bool(np.array_equal(got[0][pick][clear], (pair > top)[clear]))
    entry["kept_by_the_kernel_leg"] = int(got[0].sum())
    scale = E / len(pick)
    hip, ref = entry["hip_end_to_end_ms"], [ms * scale for ms in entry["host_pair_calls_ms"]]
    h, r = leg_summary(hip), leg_summary(ref)
    entry["summary"] = {"hip_end_to_end_mean_ms": h["mean"], "hip_spread_ms": h["spread"],
                        "host_per_pair_call_ms": leg_summary(entry["host_pair_calls_ms"])["mean"] / len(pick),
                        "host_scaled_mean_ms": r["mean"], "host_scaled_spread_ms": r["spread"],
                        "kernel_mean_ms": leg_summary(entry["kernel_ms"])["mean"],
                        "speedup_over_host": sum(ref) / sum(hip),
                        "beats_host_by_more_than_its_spread": beats(hip, ref)}
    return entry


def main():
    a = frame.arguments("host_edges", "edge_select_knn.json")
    if a.child:
        import scipy
        with switched(KN, "ENABLED", True):
            return frame.run_shape(os.path.basename(__file__), a.child,
                                   lambda n, n_edges: KN.edge_select_knn(*make_fold(n, n_edges), 1.0, K),
                                   lambda *shape: bench_shape(*shape, a.host_edges, a.warmup, a.iters, a.repeats), (np, scipy))
    result = {"workload": "valid_pca_mutual_info under --knn_mutual_info for every PPI edge of a fold (kraskov_mi of the two "
                          "raw end columns and of each end column against the label, k = 5, fp64): edge_select_knn on the "
                          "kernel of csrc/kraskov_mi.hip (MLGNN_EDGE_KNN_FUSED=1) against kraskov_mi_host (three cKDTree "
                          "per call), same input",
              "timing": "one child process per shape under a limit of %g s; in it wall clock around each call with a "
                        "device synchronise, the two legs alternating over %d repeats; the kernel alone by device events, "
                        "mean of %d launches after %d; one untimed call of the kernel leg first"
                        % (a.step_limit, a.repeats, a.iters, a.warmup)}
    frame.drive(__file__, a, "host_edges", result, "beats_host_by_more_than_its_spread")


if __name__ == "__main__":
    main()
