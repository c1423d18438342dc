#!/usr/bin/env python3
"""The mutual-information gene mask (``generate_mutual_mask`` of the models: ``mutual_info_classif`` over every gene
column) at the shapes of the shipped configurations,

  (N, F, k) = (200, 15405, 7)    gbm
              (200, 15405, 15)   lgg
              (300, 25015, 15)   kirc

on synthetic fp32 data with a planted signal (column f shifted by ``label * 2 f / F``), two labels at 70 % / 30 %.
Times ``mlgnn.mutual_info_classif`` (csrc/mutual_info.hip) against the scikit-learn call as the models make it (one job):
the two legs alternate over three repeats, so the scikit-learn leg's own spread is on record.  Reported per shape:

  * end to end, wall clock: host preparation + upload + transpose + kernel + download;
  * the kernel alone, by device events (mean of ``--iters`` launches after ``--warmup``);
  * the host preparation alone (``check_X_y``, ``scale``, the noise draw), wall clock;
  * the scikit-learn call, wall clock;
  * that both legs agree (max |difference|; both use the same ``random_state``).

The first shape is run once untimed on the op's leg before the sweep (the first launch of a process carries the load of
its code object).  Results are written after every shape.  Writes profiles/mutual_info.json.  Development tool; run it
under a time limit of its own (``timeout -k 10 900 python tools/bench_mutual_info.py``).

``--regression``: the same protocol for ``mlgnn.mutual_info_regression`` (csrc/mutual_info_cc.hip, the Kraskov estimator)
against scikit-learn's ``mutual_info_regression`` at the same shapes, with the target ``generate_mutual_mask`` hands over
when ``mutual_classif`` is false: the two-valued label as float.  Writes profiles/mutual_info_regression.json."""
import argparse
import json
import os
import sys

import numpy as np
import torch

from _bench import beats, event_ms, leg_summary, need_gpu, wall, write_json

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multilevel-gnn_amd"))
from mlgnn import _lib  # noqa: E402
from mlgnn import mutual_info as MI  # noqa: E402

SHAPES = [("gbm", 200, 15405, 7), ("lgg", 200, 15405, 15), ("kirc", 300, 25015, 15)]
REPEATS = 3
SEED = 12345


def make_data(n, F, seed):
    rng = np.random.RandomState(seed)
    y = (np.arange(n) < int(0.3 * n)).astype(np.int64)
    rng.shuffle(y)
    x = rng.standard_normal((n, F)) + y[:, None] * (2.0 * np.arange(F) / F)[None, :]
    return x.astype(np.float32), y


def kernel_ms(prepared, y, k, warmup, iters):
    """The launch of mlgnn_mutual_info_cd alone, operands resident on the device."""
    from scipy.special import digamma
    n, F = prepared.shape
    dev = torch.device("cuda:0")
    _, d, c = np.unique(y, return_inverse=True, return_counts=True)
    base = float(digamma(n) + np.mean(digamma(np.minimum(k, c[d] - 1))) - np.mean(digamma(c[d])))
    xt = torch.from_numpy(prepared).to(dev).t().contiguous()
    labels, psi_d = torch.from_numpy(d.astype(np.int32)).to(dev), torch.from_numpy(MI.digamma_table(n)).to(dev)
    mi = torch.empty(F, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def launch():
        _lib.check(_lib.lib.mlgnn_mutual_info_cd(xt.data_ptr(), labels.data_ptr(), psi_d.data_ptr(), base, mi.data_ptr(), None,
                                                 n, F, k, len(c), stream), "mlgnn_mutual_info_cd")

    return event_ms(launch, warmup, iters)


def kernel_ms_regression(prepared, y_prepared, k, warmup, iters):
    """The launch of mlgnn_mutual_info_cc alone, operands resident on the device."""
    from scipy.special import digamma
    n, F = prepared.shape
    dev = torch.device("cuda:0")
    base = float(digamma(n) + digamma(k))
    xt = torch.from_numpy(prepared).to(dev).t().contiguous()
    y_d, psi_d = torch.from_numpy(y_prepared).to(dev), torch.from_numpy(MI.digamma_table(n)).to(dev)
    mi = torch.empty(F, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def launch():
        _lib.check(_lib.lib.mlgnn_mutual_info_cc(xt.data_ptr(), y_d.data_ptr(), psi_d.data_ptr(), base, mi.data_ptr(), None,
                                                 None, n, F, k, stream), "mlgnn_mutual_info_cc")

    return event_ms(launch, warmup, iters)


def bench_shape_regression(name, n, F, k, warmup, iters, repeats):
    from sklearn.feature_selection import mutual_info_regression as sk_regression
    x, labels = make_data(n, F, 7)
    y = labels.astype(np.float64)                                             # what train.py passes
    assert MI.mutual_info_regression_supported(n, F, k), (n, F, k)
    entry = {"shape": name, "N": n, "F": F, "k": k, "label_counts": [int(c) for c in MI.label_counts(labels)],
             "hip_end_to_end_ms": [], "sklearn_ms": [], "prepare_ms": [], "kernel_ms": []}
    got = want = None
    for _ in range(repeats):                                                  # the legs alternate
        ms, got = wall(lambda: MI.mutual_info_regression(x, y, n_neighbors=k, random_state=SEED))
        entry["hip_end_to_end_ms"].append(ms)
        ms, want = wall(lambda: sk_regression(x, y, n_neighbors=k, random_state=SEED))
        entry["sklearn_ms"].append(ms)
        ms, (prepared, y_prepared) = wall(lambda: MI.prepare_regression(x, y, SEED))
        entry["prepare_ms"].append(ms)
        entry["kernel_ms"].append(kernel_ms_regression(prepared, y_prepared, k, warmup, iters))
    return compared(entry, got, want)


def bench_shape(name, n, F, k, warmup, iters, repeats):
    from sklearn.feature_selection import mutual_info_classif as sk_classif
    x, y = make_data(n, F, 7)
    counts = MI.label_counts(y)
    assert MI.mutual_info_supported(n, F, k, counts) and MI.tree_path(k, counts), (n, F, k, counts)
    entry = {"shape": name, "N": n, "F": F, "k": k, "label_counts": [int(c) for c in counts],
             "hip_end_to_end_ms": [], "sklearn_ms": [], "prepare_ms": [], "kernel_ms": []}
    got = want = None
    for _ in range(repeats):                                                  # the legs alternate
        ms, got = wall(lambda: MI.mutual_info_classif(x, y, n_neighbors=k, random_state=SEED))
        entry["hip_end_to_end_ms"].append(ms)
        ms, want = wall(lambda: sk_classif(x, y, n_neighbors=k, random_state=SEED))
        entry["sklearn_ms"].append(ms)
        ms, (prepared, _) = wall(lambda: MI.prepare(x, y, SEED))
        entry["prepare_ms"].append(ms)
        entry["kernel_ms"].append(kernel_ms(prepared, y, k, warmup, iters))
    return compared(entry, got, want)


def compared(entry, got, want):
    """``entry`` with the agreement of the two legs and its summary."""
    entry["max_abs_diff_to_sklearn"] = float(np.abs(got - want).max())
    entry["masks_equal_at_the_mean_threshold"] = bool(np.array_equal(got < got.mean(), want < want.mean()))
    hip, ref = entry["hip_end_to_end_ms"], entry["sklearn_ms"]
    h, r = leg_summary(hip), leg_summary(ref)
    entry["summary"] = {"hip_end_to_end_mean_ms": h["mean"], "hip_spread_ms": h["spread"],
                        "sklearn_mean_ms": r["mean"], "sklearn_spread_ms": r["spread"],
                        "prepare_mean_ms": leg_summary(entry["prepare_ms"])["mean"],
                        "kernel_mean_ms": leg_summary(entry["kernel_ms"])["mean"],
                        "speedup_over_sklearn": sum(ref) / sum(hip),
                        "beats_sklearn_by_more_than_its_spread": beats(hip, ref)}
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=REPEATS)
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--regression", action="store_true",
                    help="mutual_info_regression (csrc/mutual_info_cc.hip) instead of mutual_info_classif")
    ap.add_argument("--out", default=None, help="default: profiles/mutual_info.json, with --regression "
                                                "profiles/mutual_info_regression.json")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "mutual_info_regression.json" if a.regression else "mutual_info.json")
    need_gpu("bench_mutual_info.py", "CPU path of the op")
    import scipy
    import sklearn
    workload = ("mutual_info_regression over every gene column (generate_mutual_mask with mutual_classif false; the "
                "target is the two-valued label as float), fp64: the op of csrc/mutual_info_cc.hip (MLGNN_MI_REG_FUSED=1) "
                "against the scikit-learn call, same input and random_state") if a.regression else \
        ("mutual_info_classif over every gene column (generate_mutual_mask), fp64: the op of "
         "csrc/mutual_info.hip against the scikit-learn call (MLGNN_MI_FUSED=0), same input and random_state")
    result = {"workload": workload,
              "timing": "wall clock around each call with a device synchronise, the two legs alternating over %d repeats, "
                        "one process; the kernel alone by device events, mean of %d launches after %d" % (a.repeats, a.iters,
                                                                                                        a.warmup),
              "device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(),
              "versions": {"sklearn": sklearn.__version__, "numpy": np.__version__, "scipy": scipy.__version__},
              "shapes": []}
    x, y = make_data(SHAPES[0][1], 512, 1)
    if a.regression:                                                               # discarded: the code object loads
        MI.mutual_info_regression(x, y.astype(np.float64), n_neighbors=SHAPES[0][3], random_state=SEED)
    else:
        MI.mutual_info_classif(x, y, n_neighbors=SHAPES[0][3], random_state=SEED)
    for name, n, F, k in SHAPES:
        if name not in a.shapes.split(","):
            continue
        entry = (bench_shape_regression if a.regression else bench_shape)(name, n, F, k, a.warmup, a.iters, a.repeats)
        result["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        # (the regression switch ships as 0 whatever the timing: mlgnn/mutual_info.py, next to DEFAULT_REG_ENABLED)
        verdict = "beats_sklearn_at_every_shape" if a.regression else "ships_enabled"
        result[verdict] = all(e["summary"]["beats_sklearn_by_more_than_its_spread"] for e in result["shapes"]) \
            and len(result["shapes"]) == len(SHAPES)
        write_json(a.out, result)


if __name__ == "__main__":
    main()
