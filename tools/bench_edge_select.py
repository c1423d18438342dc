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
tool; run it under a time limit of its own (``timeout -k 10 600 python tools/bench_edge_select.py``)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multilevel-gnn_amd"))
from mlgnn import _lib  # noqa: E402
from mlgnn.data import SyntheticTCGA  # noqa: E402

ES = importlib.import_module("mlgnn.edge_select")
SHAPES = [("gbm", 200, 60000), ("kirc", 300, 60000)]
SEED, K = 12345, 3


def make_fold(n, n_edges):
    """``(values [n, 3 node_num] fp32, labels [n], PPI edge_index [2, E'])`` of a cohort of ``n`` training patients."""
    data = SyntheticTCGA(n, n_edges=n_edges, seed=0)
    y = (torch.arange(n) < int(0.3 * n)).long()[torch.randperm(n, generator=torch.Generator().manual_seed(1))]
    strength = 0.2 + 0.8 * torch.rand(data.NN, generator=torch.Generator().manual_seed(2))
    x = data.x[:, :, 0] + y[:, None].float() * strength[None, :]
    return x, y.numpy(), data.edge_index[:, data.n_cross:].numpy()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def kernel_ms(x, y, ei, warmup, iters):
    """The launch of mlgnn_edge_mi alone (E pairs + U singles), operands resident on the device."""
    from scipy.special import digamma
    from sklearn.utils import check_random_state
    n, n_nodes = x.shape
    dev = torch.device("cuda:0")
    nodes = np.unique(ei)
    pairs = np.concatenate([ei.T, np.stack([nodes, np.full_like(nodes, -1)], axis=1)]).astype(np.int32)
    _, d, c = np.unique(y, return_inverse=True, return_counts=True)
    psi = np.zeros(n + 1)
    psi[1:] = digamma(np.arange(1, n + 1))
    base = float(digamma(n) + np.mean(digamma(np.minimum(K, c[d] - 1))) - np.mean(digamma(c[d])))
    xt = x.to(dev).double().t().contiguous()
    ops = [torch.from_numpy(a).to(dev) for a in (pairs, check_random_state(SEED).standard_normal(n), d.astype(np.int32), psi)]
    mi = torch.zeros(len(pairs), dtype=torch.float64, device=dev)

    def launch():
        _lib.call("mlgnn_edge_mi", xt, ops[0], ops[1], ops[2], ops[3], base, mi, None, None, n, n_nodes, len(pairs), K,
                  len(c), _lib.stream())

    for _ in range(warmup):
        launch()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        launch()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters, len(pairs)


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
        ES.ENABLED = True
        ms, got = wall(lambda: ES.edge_select(x, y, ei, 1.0, K, SEED))
        entry["hip_end_to_end_ms"].append(ms)
        ES.ENABLED = False
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
    entry["summary"] = {"hip_end_to_end_mean_ms": sum(hip) / repeats, "hip_spread_ms": max(hip) - min(hip),
                        "sklearn_per_edge_ms": sum(entry["sklearn_subsample_ms"]) / repeats / len(pick),
                        "sklearn_scaled_mean_ms": sum(ref) / repeats, "sklearn_scaled_spread_ms": max(ref) - min(ref),
                        "kernel_mean_ms": sum(entry["kernel_ms"]) / repeats,
                        "speedup_over_sklearn": sum(ref) / sum(hip),
                        "beats_sklearn_by_more_than_its_spread": sum(ref) / repeats - sum(hip) / repeats > max(ref) - min(ref)}
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sklearn_edges", type=int, default=400)
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_select.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_edge_select.py needs the GPU: there is no CPU path of the op to time")
    import scipy
    import sklearn
    was = ES.ENABLED
    result = {"workload": "valid_pca_mutual_info for every PPI edge of a fold (PCA(n_components=1) of the two end columns, "
                          "mutual_info_classif of its score and of each end column, fp64): edge_select on the kernel of "
                          "csrc/edge_select.hip (MLGNN_EDGE_SELECT_FUSED=1) against the loop of scikit-learn calls, same "
                          "input and random_state",
              "timing": "wall clock around each call with a device synchronise, the two legs alternating over %d repeats, "
                        "one process; the kernel alone by device events, mean of %d launches after %d; one untimed call "
                        "of the kernel leg first" % (a.repeats, a.iters, a.warmup),
              "device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(),
              "versions": {"sklearn": sklearn.__version__, "numpy": np.__version__, "scipy": scipy.__version__},
              "shapes": []}
    x, y, ei = make_fold(SHAPES[0][1], 2000)
    ES.ENABLED = True
    ES.edge_select(x, y, ei, 1.0, K, SEED)                                         # discarded: the code object loads
    for name, n, n_edges in SHAPES:
        if name not in a.shapes.split(","):
            continue
        entry = bench_shape(name, n, n_edges, a.sklearn_edges, a.warmup, a.iters, a.repeats)
        result["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        result["ships_enabled"] = all(e["summary"]["beats_sklearn_by_more_than_its_spread"] for e in result["shapes"]) \
            and len(result["shapes"]) == len(SHAPES)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
    ES.ENABLED = was


if __name__ == "__main__":
    main()
