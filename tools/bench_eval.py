#!/usr/bin/env python3
"""The evaluation pass of an epoch (the mean BCE loss of the batches, accuracy, ROC AUC) on device-resident predictions:

  cohorts of N = 200, 300, 470 patients in the reference's 5-fold scheme -- test ``N // 5``, valid ``(N - test) // 5``,
  train the rest -- as one 3-row call at batch sizes 32 and 64, and per cohort one pooled row of the whole cohort.

Times ``EvalBuffer.finish()`` on the kernel of csrc/eval_metrics.hip against ``binary_metrics_host`` plus the download it
needs -- the lines ``train_harness.evaluate`` ran before the kernel existed -- in one process, both legs on the same
device-resident ``pred`` and ``y``.  Per shape:

  * one untimed call of each leg, then the two legs alternating over ``--repeats`` repeats, wall clock with a device
    synchronise on either side, the garbage collector held off;
  * the launch alone, by device events (mean of ``--iters`` calls of the entry point after ``--warmup``);
  * that the two legs agree: accuracy and counts equal, AUC within ``(n + 8) 2^-53``, loss within 1e-4.

Every shape runs in a child process of its own under a time limit (``--step-timeout``); the first one that fails or runs
out of time ends the run (``drive`` of tools/_bench.py).  Writes profiles/eval_metrics.json, whose ``ships_enabled`` is the
rule for the default of ``MLGNN_EVAL_FUSED``: the kernel leg beats the host leg by more than that leg's spread at every
shape measured.  Development tool; run it under a time limit of its own."""
import argparse
import gc
import json
import os
import sys

from _bench import alternate, beats, child_result, drive, event_ms, leg_summary, need_gpu, switched, wall, write_json  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multilevel-gnn_amd"))

PATIENTS = (200, 300, 470)
BATCH_SIZES = (32, 64)
REPEATS = 3
SEED = 0


def split_rows(n):
    """The reference's 5-fold scheme (train.py:253-255) -> ``[train, valid, test]``."""
    test = n // 5
    valid = (n - test) // 5
    return [n - test - valid, valid, test]


def shapes():
    """name -> (rows, batch size)."""
    out = {}
    for n in PATIENTS:
        for b in BATCH_SIZES:
            out["N%d_splits_b%d" % (n, b)] = (split_rows(n), b)
        out["N%d_pooled" % n] = ([n], n)
    return out


def batches_of(n, size):
    return [size] * (n // size) + ([n % size] if n % size else [])


def launch_ms(M, pred, y, rows, batch_sizes, warmup, iters):
    """The one launch of mlgnn_eval_metrics alone, everything resident on the device."""
    import torch
    from mlgnn import _lib
    pointers, n_batches = M._pointers(rows, batch_sizes)
    n_rows = len(rows)
    ptrs = torch.tensor(pointers, dtype=torch.int32, device=pred.device)
    row_ptr, batch_ptr, row_batch_ptr = ptrs[:n_rows + 1], ptrs[n_rows + 1:n_rows + n_batches + 2], ptrs[n_rows + n_batches + 2:]
    out_f64 = torch.zeros((n_rows, 3), dtype=torch.float64, device=pred.device)
    out_i64 = torch.zeros((n_rows, 6), dtype=torch.int64, device=pred.device)

    def launch():
        _lib.call("mlgnn_eval_metrics", pred, y, row_ptr, batch_ptr, row_batch_ptr, n_rows, max(rows), int(pred.shape[0]),
                  n_batches, out_f64, out_i64, None, 0, _lib.stream())

    return event_ms(launch, warmup, iters)


def run_shape(rows, batch, repeats, warmup, iters):
    import torch
    from mlgnn import metrics as M
    need_gpu("bench_eval.py", "CPU path of the op")
    dev = torch.device("cuda")
    total = sum(rows)
    g = torch.Generator().manual_seed(SEED)
    label = (torch.rand(total, generator=g) < 0.3).to(torch.float32)
    p = (0.3 * label + 0.7 * torch.rand(total, generator=g)).clamp(0.01, 0.99)     # scores that carry some signal
    pred_h, y_h = torch.stack([p, 1 - p], 1), torch.stack([label, 1 - label], 1)
    batch_sizes = [batches_of(n, batch) for n in rows]
    buf = M.EvalBuffer(total, dev)

    def fill():
        at = 0
        for n, sizes in zip(rows, batch_sizes):
            for b in sizes:
                buf.append(pred_h[at:at + b].to(dev), y_h[at:at + b].to(dev))
                at += b
            buf.close_row()

    pred, y = buf.pred, buf.y                                      # both legs read these

    def kernel_leg(_):
        fill()                                                     # (outside the clock: both legs start from the buffer)
        with switched(M, "ENABLED", True):
            return wall(buf.finish)

    def host_leg(_):
        fill()
        buf.reset()
        return wall(lambda: M.binary_metrics_host(pred[:total], y[:total], batch_sizes, rows))

    results = {}

    def keep(name, leg):
        def measure(arg):
            ms, res = leg(arg)
            results.setdefault(name, []).append(res)
            return ms
        return measure

    kernel_leg(None)                                               # discarded: the code object loads
    host_leg(None)                                                 # discarded: the first download sets up its staging
    before = dict(M.EVAL_STATS)
    gc.collect()
    gc.disable()                                                   # (as timeit does: no collection inside a timed call)
    # `alternate` hands each measure its leg's argument: the legs themselves are the arguments here
    timed = alternate(repeats, {"hip": keep("hip", kernel_leg), "host": keep("host", host_leg)}, {"ms": lambda fn: fn(None)})
    gc.enable()
    runs = {leg: timed[leg]["ms"] for leg in timed}
    assert M.EVAL_STATS == dict(hip=before["hip"] + repeats, host=before["host"]), M.EVAL_STATS

    agree = True
    for got, want in zip(results["hip"], results["host"]):
        for a, b in zip(got, want):
            agree &= (a.n, a.n_pos, a.n_correct, a.acc) == (b.n, b.n_pos, b.n_correct, b.acc)
            agree &= abs(a.auc - b.auc) <= (a.n + 8) * 2.0 ** -53
            agree &= abs(a.loss - b.loss) <= 1e-4 * max(1.0, abs(b.loss))
    fill()
    buf.reset()
    return {"hip_ms": runs["hip"], "host_with_download_ms": runs["host"],
            "kernel_ms": launch_ms(M, pred[:total], y[:total], rows, batch_sizes, warmup, iters), "legs_agree": bool(agree),
            "device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads()}


def with_summary(entry):
    hip, ref = entry["hip_ms"], entry["host_with_download_ms"]
    h, r = leg_summary(hip), leg_summary(ref)
    entry["summary"] = {"hip_mean_ms": h["mean"], "hip_spread_ms": h["spread"], "host_with_download_mean_ms": r["mean"],
                        "host_with_download_spread_ms": r["spread"], "speedup_over_host": sum(ref) / sum(hip),
                        "beats_host_by_more_than_its_spread": beats(hip, ref)}
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=REPEATS)
    ap.add_argument("--step-timeout", type=float, default=60.0, help="seconds, per shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_metrics.json"))
    ap.add_argument("--child", default=None, help="(internal) run this shape and print its result line")
    a = ap.parse_args()
    by_name = shapes()
    if a.child:
        return child_result(run_shape(*by_name[a.child], a.repeats, a.warmup, a.iters))
    import sklearn
    result = {"workload": "the evaluation pass (mean BCE loss of the batches, accuracy, ROC AUC) of the three splits of the "
                          "reference's 5-fold scheme as one 3-row call, and of one pooled row per cohort: "
                          "EvalBuffer.finish() on the kernel of csrc/eval_metrics.hip against binary_metrics_host "
                          "(MLGNN_EVAL_FUSED=0) plus the download it needs, both from the same device-resident buffers",
              "timing": "wall clock around each call with a device synchronise on either side, the legs alternating over %d "
                        "repeats, one untimed call of each leg first, no garbage collection inside; every shape a fresh "
                        "process under a limit of %g s; the launch alone by device events, mean of %d calls after %d"
                        % (a.repeats, a.step_timeout, a.iters, a.warmup),
              "versions": {"scikit-learn": sklearn.__version__}, "shapes": []}

    def collect(name, step):
        rows, batch = by_name[name]
        entry = {"shape": name, "rows": rows, "batch_size": batch}
        for key in ("device", "host_threads"):
            result[key] = step.pop(key)
        entry.update(step)
        result["shapes"].append(with_summary(entry))
        print(json.dumps(entry), flush=True)
        result["ships_enabled"] = len(result["shapes"]) == len(by_name) and all(
            e["summary"]["beats_host_by_more_than_its_spread"] and e["legs_agree"] for e in result["shapes"])

    drive(__file__, list(by_name), ["--warmup", a.warmup, "--iters", a.iters, "--repeats", a.repeats], a.step_timeout, a.out,
          result, collect)


if __name__ == "__main__":
    main()
