#!/usr/bin/env python3
"""The ``--edge_select`` test of the fold preparation with ``mutual_classif`` false (``valid_pca_mutual_info`` under
``mutual_info_regression``, the reference's default) at the ``(n, E)`` of the gbm and kirc training folds on
:class:`mlgnn.data.SyntheticTCGA`,

  (n, E) = (200, 60000)   gbm
           (300, 60000)   kirc

with the label planted in every node, as in tools/bench_edge_select.py, whose protocol this follows: wall clock with a
device synchronise, the legs alternating over three repeats so the host leg's spread is on record, the kernel alone by
device events, one untimed call first.  Times ``mlgnn.edge_select_reg.edge_select_regression`` on the kernel of
csrc/edge_select_cc.hip -- in both of its forms: one launch (both states the same seed) and two launches (the pair calls
unseeded, what the fold preparation runs) -- against the reference's scikit-learn calls (``PCA(n_components=1)`` and
``mutual_info_regression``, three KD-trees per call).  The host leg runs on a fixed subsample of ``--host_edges`` edges (the
whole fold takes minutes); its time is scaled to ``E`` at the PAIR calls alone -- the subsample's end-node calls are timed
apart and left out, since the whole fold computes each end node once: a lower bound of the loop's time -- and the JSON says
so.  Both legs' values and decisions are compared on the subsample, seeded alike.

``ships_enabled`` is the rule for the default of ``MLGNN_EDGE_REG_FUSED``: the kernel leg on ALL edges, in the slower of
its two forms, beats the scaled host leg by more than that leg's scaled spread at both shapes.  Writes
profiles/edge_select_reg.json.  Development tool; every shape runs in a fresh child process under ``--step_limit``
(``drive`` of tools/_bench.py)."""
import importlib
import os

import numpy as np

import _edge_bench as frame
from _bench import beats, leg_summary, switched, wall

ER = importlib.import_module("mlgnn.edge_select_reg")
SEED, K = 12345, 3


def make_fold(n, n_edges):
    return frame.make_fold(n, n_edges, np.float64)


def kernel_ms(x, y, ei, warmup, iters):
    """The launch of mlgnn_edge_mi_cc alone (E pairs + U singles), operands resident on the device."""
    from scipy.special import digamma
    return frame.kernel_ms("mlgnn_edge_mi_cc", x, ei, ER.prepare_target(y, SEED), digamma(len(y)) + digamma(K), K, 3, (),
                           warmup, iters)


def host_pair_calls(x, y, pairs):
    """The reference's pair calls: PCA(n_components=1) on the two end columns, mutual_info_regression of its score."""
    from sklearn.decomposition import PCA
    from sklearn.feature_selection import mutual_info_regression
    out = np.zeros(len(pairs))
    for e, (s, t) in enumerate(pairs.tolist()):
        edge_data = x[:, [s, t]]
        pca_data = PCA(n_components=1).fit(edge_data).transform(edge_data)
        out[e] = mutual_info_regression(pca_data, y, n_neighbors=K, random_state=SEED)[0]
    return out


def host_node_calls(x, y, nodes):
    from sklearn.feature_selection import mutual_info_regression
    return np.array([mutual_info_regression(x[:, v][:, None], y, n_neighbors=K, random_state=SEED)[0] for v in nodes.tolist()])


def bench_shape(name, n, n_edges, sub, warmup, iters, repeats):
    x, y, ei = make_fold(n, n_edges)
    E = ei.shape[1]
    pick = np.random.RandomState(3).choice(E, size=min(sub, E), replace=False)
    x_host = x.numpy().astype(np.float64)
    singles = np.unique(ei[:, pick])
    entry = {"shape": name, "n": n, "E": E, "n_nodes": int(x.shape[1]), "k": K, "host_edges": int(len(pick)),
             "host_leg": "the reference's scikit-learn calls on a fixed subsample of the edges; scaled to E at the PAIR "
                         "calls alone (the subsample's end-node calls are timed apart and left out: the whole fold computes "
                         "each end node once): a lower bound of the loop's time",
             "hip_end_to_end_ms": [], "hip_two_launches_ms": [], "host_pair_calls_ms": [], "host_node_calls_ms": [],
             "kernel_ms": []}
    got = pair = node = None
    for _ in range(repeats):                                                  # the legs alternate
        ms, got = wall(lambda: ER.edge_select_regression(x, y, ei, 1.0, K, SEED, SEED))
        entry["hip_end_to_end_ms"].append(ms)
        ms, _ = wall(lambda: ER.edge_select_regression(x, y, ei, 1.0, K, SEED, None))
        entry["hip_two_launches_ms"].append(ms)
        ms, pair = wall(lambda: host_pair_calls(x_host, y, ei[:, pick].T))
        entry["host_pair_calls_ms"].append(ms)
        ms, node = wall(lambda: host_node_calls(x_host, y, singles))
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
    one, two = entry["hip_end_to_end_ms"], entry["hip_two_launches_ms"]
    hip = one if sum(one) >= sum(two) else two                                 # the slower form decides
    ref = [ms * scale for ms in entry["host_pair_calls_ms"]]
    h1, h2, r = leg_summary(one), leg_summary(two), leg_summary(ref)
    entry["summary"] = {"hip_end_to_end_mean_ms": h1["mean"], "hip_spread_ms": h1["spread"],
                        "hip_two_launches_mean_ms": h2["mean"], "hip_two_launches_spread_ms": h2["spread"],
                        "host_per_pair_call_ms": leg_summary(entry["host_pair_calls_ms"])["mean"] / len(pick),
                        "host_scaled_mean_ms": r["mean"], "host_scaled_spread_ms": r["spread"],
                        "kernel_mean_ms": leg_summary(entry["kernel_ms"])["mean"],
                        "speedup_over_host": sum(ref) / sum(hip),
                        "beats_host_by_more_than_its_spread": beats(hip, ref)}
    return entry


def main():
    a = frame.arguments("host_edges", "edge_select_reg.json")
    if a.child:
        import scipy
        import sklearn
        with switched(ER, "ENABLED", True):
            return frame.run_shape(os.path.basename(__file__), a.child,
                                   lambda n, n_edges: ER.edge_select_regression(*make_fold(n, n_edges), 1.0, K, SEED, SEED),
                                   lambda *shape: bench_shape(*shape, a.host_edges, a.warmup, a.iters, a.repeats),
                                   (sklearn, np, scipy))
    result = {"workload": "valid_pca_mutual_info with mutual_classif false for every PPI edge of a fold "
                          "(PCA(n_components=1) of the two end columns, mutual_info_regression of its score and of each end "
                          "column against the label, k = 3, fp64): edge_select_regression on the kernel of "
                          "csrc/edge_select_cc.hip (MLGNN_EDGE_REG_FUSED=1) against the scikit-learn calls, same input and "
                          "seeds",
              "timing": "one child process per shape under a limit of %g s; in it wall clock around each call with a "
                        "device synchronise, the two legs alternating over %d repeats; the kernel alone by device events, "
                        "mean of %d launches after %d; one untimed call of the kernel leg first"
                        % (a.step_limit, a.repeats, a.iters, a.warmup)}
    frame.drive(__file__, a, "host_edges", result, "beats_host_by_more_than_its_spread")


if __name__ == "__main__":
    main()
