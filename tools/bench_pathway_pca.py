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
first step that fails ends the run.  Results are written after every step.  Writes profiles/pathway_pca.json, whose
``ships_enabled`` is the rule for the default of ``MLGNN_PCA_FUSED``: the kernel leg beats the scikit-learn leg by more
than that leg's spread at the masked N = 300 and N = 470 shapes.  Development tool; run it under a time limit of its own
(``timeout -k 10 900 python tools/bench_pathway_pca.py``)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multilevel-gnn_amd"))

PATIENTS = (200, 300, 470)
REPEATS = 3
SEED = 0


def shapes():
    return [(n, masked, sim) for n in PATIENTS for masked in (False, True) for sim in (2, 3)]


def shape_name(n, masked, sim):
    return "N%d_%s_sim%d" % (n, "masked" if masked else "unmasked", sim)


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


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

    for _ in range(warmup):
        launch()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        launch()
    e.record()
    torch.cuda.synchronize()
    info = outs[4].cpu().numpy()
    return s.elapsed_time(e) / iters, int(info[:, 0].max()), int((info[:, 0] < 0).sum())


def run_step(n, masked, sim, warmup, iters):
    """One repeat of one shape, in this process: an untimed kernel-leg call, then the two legs, then the kernel alone."""
    import numpy as np
    import torch
    import mlgnn
    from mlgnn import pca as P
    from mlgnn.data import SyntheticTCGA
    if not torch.cuda.is_available():
        raise SystemExit("bench_pathway_pca.py needs the GPU: there is no CPU path of the op to time")
    data = SyntheticTCGA(n, seed=SEED)
    raw = data.raw_matrix()                                        # fp32 [N, 25015] on the host, as the harness has it
    mask = None
    if masked:
        mi = mlgnn.mutual_info_classif(raw.numpy(), data.labels.numpy(), n_neighbors=3, random_state=12345)
        mask = torch.from_numpy((mi >= mi.mean()).astype(np.float32))[:, None]
    pca_dim = 2

    def leg(enabled):
        P.ENABLED = enabled
        return P.fold_pca(raw, data.raw_indice, mask, sim, pca_dim)

    leg(True)                                                      # discarded: the code object loads
    before = dict(P.PCA_STATS)
    hip_ms, got = wall(lambda: leg(True))
    ref_ms, want = wall(lambda: leg(False))
    assert P.PCA_STATS == dict(hip=before["hip"] + 1, sklearn=before["sklearn"] + 1), P.PCA_STATS
    plan = P.FoldPlan(data.raw_indice, mask, sim, 438)
    k_ms, sweeps, capped = kernel_ms(raw, plan, sim, warmup, iters)
    return {"hip_end_to_end_ms": hip_ms, "sklearn_ms": ref_ms, "kernel_ms": k_ms, "max_sweeps": sweeps,
            "segments_at_the_sweep_cap": capped, "members_kept": int(plan.sizes.sum()),
            "largest_segment": int(plan.sizes.max()),
            "components_max_abs_diff": float((got[0] - want[0]).abs().max()),
            "image_max_abs_diff": float((got[1] - want[1]).abs().max()),
            "device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads()}


def summarise(entry):
    hip, ref = entry["hip_end_to_end_ms"], entry["sklearn_ms"]
    r = len(hip)
    entry["summary"] = {"hip_end_to_end_mean_ms": sum(hip) / r, "hip_spread_ms": max(hip) - min(hip),
                        "sklearn_mean_ms": sum(ref) / r, "sklearn_spread_ms": max(ref) - min(ref),
                        "kernel_mean_ms": sum(entry["kernel_ms"]) / r, "speedup_over_sklearn": sum(ref) / sum(hip),
                        "beats_sklearn_by_more_than_its_spread": sum(ref) / r - sum(hip) / r > max(ref) - min(ref)}
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=REPEATS)
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds, per repeat of a shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pathway_pca.json"))
    ap.add_argument("--step", default=None, help="(internal) N,masked,sim: run one repeat and print its JSON line")
    a = ap.parse_args()
    if a.step:
        n, masked, sim = (int(v) for v in a.step.split(","))
        print("STEP " + json.dumps(run_step(n, bool(masked), sim, a.warmup, a.iters)), flush=True)
        return
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
    for n, masked, sim in shapes():
        entry = {"shape": shape_name(n, masked, sim), "N": n, "masked": masked, "pca_sim_dim": sim,
                 "hip_end_to_end_ms": [], "sklearn_ms": [], "kernel_ms": []}
        for _ in range(a.repeats):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", "%d,%d,%d" % (n, int(masked), sim),
                   "--warmup", str(a.warmup), "--iters", str(a.iters)]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
            lines = [ln for ln in out.stdout.splitlines() if ln.startswith("STEP ")]
            if out.returncode != 0 or len(lines) != 1:
                sys.stderr.write(out.stdout + out.stderr)
                raise SystemExit("step %s failed with status %d: nothing more is started" % (entry["shape"], out.returncode))
            step = json.loads(lines[0][5:])
            for key in ("hip_end_to_end_ms", "sklearn_ms", "kernel_ms"):
                entry[key].append(step.pop(key))
            for key in ("device", "host_threads"):
                result[key] = step.pop(key)
            for key, v in step.items():
                entry[key] = max(entry.get(key, v), v)
        result["shapes"].append(summarise(entry))
        print(json.dumps(entry), flush=True)
        decisive = [e for e in result["shapes"] if e["masked"] and e["N"] in (300, 470)]
        result["ships_enabled"] = len(decisive) == 4 and all(e["summary"]["beats_sklearn_by_more_than_its_spread"]
                                                             for e in decisive)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
