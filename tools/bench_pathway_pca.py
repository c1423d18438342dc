#!/usr/bin/env python3
"""The per-fold pathway PCA (``recalculate_pca_bo_selected_gene``: one PCA per (pathway, omics) segment over the members
the mutual-information mask kept) on ``SyntheticTCGA``'s segment table -- 25 015 members, 438 segments -- at

  N = 200, 300, 470 patients;  unmasked and under the mean-threshold mask of the cohort's planted signal
  (``mutual_info_classif`` of the members against the label, threshold at the mean);  ``pca_sim_dim`` 2 and 3.

Times ``mlgnn.pca.fold_pca`` on the kernel of csrc/pathway_pca.hip against ``fold_pca`` with the switch off (the loop of
438 scikit-learn fits) in the same process: the two legs alternate, one untimed call of the kernel leg first.  Reported
per shape and repeat:

  * both legs end to end, wall clock with a device synchronise: host tables + upload + upcast and transpose + kernel +
    download for the kernel leg;
  * the kernel alone, by device events (mean of ``--iters`` launches after ``--warmup``), operands resident;
  * that both legs agree (max |difference| of ``pca_components`` and of the fp32 image), the largest sweep count.

Every repeat of a shape is a step of its own: a fresh child process under its own time limit (``--step-timeout``); the
first step that fails or runs out of time ends the run (``drive`` of tools/_bench.py).  Results are written after every
step.  Writes profiles/pathway_pca.json, whose
``ships_enabled`` is the rule for the default of ``MLGNN_PCA_FUSED``: the kernel leg beats the scikit-learn leg by more
than that leg's spread at the masked N = 300 and N = 470 shapes.  Development tool; run it under a time limit of its own
(``timeout -k 10 900 python tools/bench_pathway_pca.py``)."""
import argparse
import json
import os
import sys

from _bench import beats, child_result, drive, event_ms, leg_summary, need_gpu, switched, wall

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multilevel-gnn_amd"))

PATIENTS = (200, 300, 470)
REPEATS = 3
SEED = 0


def shapes():
    return [(n, masked, sim) for n in PATIENTS for masked in (False, True) for sim in (2, 3)]


def shape_name(n, masked, sim):
    return "N%d_%s_sim%d" % (n, "masked" if masked else "unmasked", sim)


def kernel_ms(raw, plan, sim, warmup, iters):
    """The launch of mlgnn_pathway_pca alone, operands resident on the device -> (ms, largest sweep count)."""
    import numpy as np
    import torch
    from mlgnn import _lib
    dev = torch.device("cuda:0")
    n, n_features = raw.shape
    total, n_seg, most = int(plan.sizes.sum()), len(plan.sizes), int(plan.sizes.max())
    xt = raw.to(dev).to(torch.float64).t().contiguous()
    f64 = dict(dtype=torch.float64, device=dev)
    outs = [torch.zeros((total, sim), **f64), torch.zeros((n, n_seg, sim), **f64), torch.zeros((n_seg, sim), **f64),
            torch.zeros(total, **f64), torch.zeros((n_seg, 2), dtype=torch.int32, device=dev)]
    need = _lib.size("mlgnn_pathway_pca_workspace_bytes", n, total, n_seg, most)
    work = torch.zeros(max(need, 1), dtype=torch.uint8, device=dev)
    cols = torch.from_numpy(plan.cols.astype(np.int32)).to(dev)
    ptr = torch.from_numpy(plan.seg_ptr).to(dev)
    ks = torch.from_numpy(plan.k_seg.astype(np.int32)).to(dev)

    def launch():
        _lib.call("mlgnn_pathway_pca", xt, cols, ptr, ks, *outs, work, need, n, n_features, total, n_seg, most, sim,
                  _lib.stream())

    ms = event_ms(launch, warmup, iters)
    info = outs[4].cpu().numpy()
    return ms, int(info[:, 0].max()), int((info[:, 0] < 0).sum())


def run_step(n, masked, sim, warmup, iters):
    """One repeat of one shape, in this process: an untimed kernel-leg call, then the two legs, then the kernel alone."""
    import numpy as np
    import torch
    import mlgnn
    from mlgnn import pca as P
    from mlgnn.data import SyntheticTCGA
    need_gpu("bench_pathway_pca.py", "CPU path of the op")
    data = SyntheticTCGA(n, seed=SEED)
    raw = data.raw_matrix()                                        # fp32 [N, 25015] on the host, as the harness has it
    mask = None
    if masked:
        mi = mlgnn.mutual_info_classif(raw.numpy(), data.labels.numpy(), n_neighbors=3, random_state=12345)
        mask = torch.from_numpy((mi >= mi.mean()).astype(np.float32))[:, None]
    pca_dim = 2

    def leg(enabled):
        """-> (ms, result): the switch is set outside the timed call."""
        with switched(P, "ENABLED", enabled):
            return wall(lambda: P.fold_pca(raw, data.raw_indice, mask, sim, pca_dim))

    leg(True)                                                      # discarded: the code object loads
    before = dict(P.PCA_STATS)
    hip_ms, got = leg(True)
    ref_ms, want = leg(False)
    assert P.PCA_STATS == dict(hip=before["hip"] + 1, sklearn=before["sklearn"] + 1), P.PCA_STATS
    plan = P.FoldPlan(data.raw_indice, mask, sim, 438)
    k_ms, sweeps, capped = kernel_ms(raw, plan, sim, warmup, iters)
    return {"hip_end_to_end_ms": hip_ms, "sklearn_ms": ref_ms, "kernel_ms": k_ms, "max_sweeps": sweeps,
            "segments_at_the_sweep_cap": capped, "members_kept": int(plan.sizes.sum()),
            "largest_segment": int(plan.sizes.max()),
            "components_max_abs_diff": float((got[0] - want[0]).abs().max()),
            "image_max_abs_diff": float((got[1] - want[1]).abs().max()),
            "device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads()}


def with_summary(entry):
    hip, ref = entry["hip_end_to_end_ms"], entry["sklearn_ms"]
    h, r = leg_summary(hip), leg_summary(ref)
    entry["summary"] = {"hip_end_to_end_mean_ms": h["mean"], "hip_spread_ms": h["spread"],
                        "sklearn_mean_ms": r["mean"], "sklearn_spread_ms": r["spread"],
                        "kernel_mean_ms": leg_summary(entry["kernel_ms"])["mean"], "speedup_over_sklearn": sum(ref) / sum(hip),
                        "beats_sklearn_by_more_than_its_spread": beats(hip, ref)}
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=REPEATS)
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds, per repeat of a shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pathway_pca.json"))
    ap.add_argument("--child", default=None, help="(internal) run one repeat of this shape and print its result line")
    a = ap.parse_args()
    by_name = {shape_name(*shape): shape for shape in shapes()}
    if a.child:
        return child_result(run_step(*by_name[a.child], a.warmup, a.iters))
    import numpy as np
    import scipy
    import sklearn
    result = {"workload": "fold_pca (the PCA of every (pathway, omics) segment of a fold, fp64) on SyntheticTCGA's segment "
                          "table, 25 015 members in 438 segments: the kernel of csrc/pathway_pca.hip against the loop of "
                          "scikit-learn fits (MLGNN_PCA_FUSED=0), same input",
              "timing": "wall clock around each call with a device synchronise, the two legs alternating, one untimed "
                        "kernel-leg call first; every repeat a fresh process under a limit of %g s; the kernel alone by "
                        "device events, mean of %d launches after %d" % (a.step_timeout, a.iters, a.warmup),
              "versions": {"sklearn": sklearn.__version__, "numpy": np.__version__, "scipy": scipy.__version__},
              "shapes": []}
    entries = {}

    def collect(name, step):
        """One repeat of shape ``name``; the shape's entry goes to the result with its last repeat."""
        n, masked, sim = by_name[name]
        entry = entries.setdefault(name, {"shape": name, "N": n, "masked": masked, "pca_sim_dim": sim,
                                          "hip_end_to_end_ms": [], "sklearn_ms": [], "kernel_ms": []})
        for key in ("hip_end_to_end_ms", "sklearn_ms", "kernel_ms"):
            entry[key].append(step.pop(key))
        for key in ("device", "host_threads"):
            result[key] = step.pop(key)
        for key, v in step.items():
            entry[key] = max(entry.get(key, v), v)
        if len(entry["kernel_ms"]) < a.repeats:
            return
        result["shapes"].append(with_summary(entry))
        print(json.dumps(entry), flush=True)
        decisive = [e for e in result["shapes"] if e["masked"] and e["N"] in (300, 470)]
        result["ships_enabled"] = len(decisive) == 4 and all(e["summary"]["beats_sklearn_by_more_than_its_spread"]
                                                             for e in decisive)

    drive(__file__, [name for name in by_name for _ in range(a.repeats)], ["--warmup", a.warmup, "--iters", a.iters],
          a.step_timeout, a.out, result, collect)


if __name__ == "__main__":
    main()
