#!/usr/bin/env python3
"""The training criterion of the supervised models (train.py:53-61: BCELoss in one of its weightings plus the pca feature
loss), fp32, at

  (B, M) = (32, 28032)   gbm : batch 32, pca_feature [32, 32, 146, 3 * 2]   (tools/bench_tcga.py)
           (64, 42048)   kirc: batch 64, pca_feature [64, 32, 146, 3 * 3]
           (64, 0)       no feature term (DeeperGCN, eval)

in modes 'plain' and 'sample'.  Times, with device events (mean of 50 runs after 10 warm-up runs, one process),
``mlgnn.train_criterion`` (csrc/criterion.hip) against the torch lines it replaces on the same tensors, forward and
forward + backward; the two legs alternate over three repeats, so the torch leg's own spread is on record.  Also counts
the device kernels each leg launches (``torch.profiler``) and checks that both legs agree.  With ``--steps K`` it also
times the gbm- and kirc-shape training step of tools/bench_tcga.py with ``TrainCriterion`` under both settings of the
switch, with the shipped flags (``pca_indep_loss`` only) and with ``pca_loss`` added.  The first shape is run once
untimed before the sweep (the first entry of a process otherwise carries its warm-up).  Writes profiles/criterion.json.
Development tool; run it under a time limit of its own (``timeout -k 10 600 python tools/bench_criterion.py``)."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch

from _bench import alternate, beats, event_ms, leg_summary, need_gpu, switched, wall, write_json

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multilevel-gnn_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mlgnn import criterion as C  # noqa: E402

SHAPES = [("gbm", 32, 28032), ("kirc", 64, 42048), ("no_feature", 64, 0)]
MODES = ["plain", "sample"]
REPEATS = 3
COEF = 1.0


def device_kernels(fn):
    """Number of device kernels one call of ``fn`` launches (copies and fills are not counted); None without a profiler."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA
                   and not ev.name.lower().startswith(("memcpy", "memset")))
    except Exception as exc:                           # noqa: BLE001
        print("torch.profiler: %r" % (exc,), file=sys.stderr)
        return None


def torch_lines(pred, y, feat, mode, cw):
    """The lines of ``TrainCriterion``'s torch path on given tensors."""
    bce = torch.nn.functional.binary_cross_entropy
    if mode == "sample":
        loss = (C._sample_weight(cw, y)[:, None] * bce(pred, y, reduction="none")).mean()
    else:
        loss = bce(pred, y)
    if feat is not None:
        loss = loss + (0 - COEF * torch.log(torch.mean(torch.std(feat.reshape(feat.shape[0], -1), dim=0))))
    return loss


def bench_shape(name, B, M, mode, dev, warmup, iters):
    torch.manual_seed(1)
    pred = torch.softmax(torch.randn(B, 2, device=dev), dim=1).requires_grad_()
    y = torch.nn.functional.one_hot(torch.randint(0, 2, (B,), device=dev), 2).float()
    feat = (0.3 * torch.randn(B, M, device=dev) + 0.5).requires_grad_() if M else None
    cw = torch.rand(B, 2, device=dev) + 0.5
    leaves = [pred] + ([feat] if M else [])
    legs = {"hip": lambda: C.train_criterion(pred, y, feat, COEF, mode, cw if mode != "plain" else None),
            "torch": lambda: torch_lines(pred, y, feat, mode, cw)}

    def step(fn):
        def run():
            for t in leaves:
                t.grad = None
            fn().backward()
        return run

    res = {}
    for leg, fn in legs.items():
        step(fn)()
        res[leg] = (float(fn()), [t.grad.clone() for t in leaves])
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
    entry = {"shape": name, "B": B, "M": M, "mode": mode,
             "mbytes_forward": (B * M + 2 * M + 4 * B) * 4 / 1e6,            # feat read once (twice from L2), colstats written
             "mbytes_backward": (2 * B * M + 2 * M + 6 * B) * 4 / 1e6,       # feat read, grad_feat written
             "agreement": {"loss_hip": res["hip"][0], "loss_torch": res["torch"][0],
                           "grad_max_abs_diff_over_max_abs": [rel(a, b) for a, b in zip(res["hip"][1], res["torch"][1])]},
             "device_kernels": {leg: {"forward": device_kernels(fn), "forward_backward": device_kernels(step(fn))}
                                for leg, fn in legs.items()}}
    entry.update(alternate(REPEATS, legs, {"forward_ms": lambda fn: event_ms(fn, warmup, iters),           # the legs alternate
                                           "forward_backward_ms": lambda fn: event_ms(step(fn), warmup, iters)}))
    entry["summary"] = {}
    for key in ("forward_ms", "forward_backward_ms"):
        hip, ref = entry["hip"][key], entry["torch"][key]
        h, r = leg_summary(hip), leg_summary(ref)
        entry["summary"][key] = {"hip_mean": h["mean"], "torch_mean": r["mean"], "torch_spread": r["spread"],
                                 "hip_spread": h["spread"], "speedup_over_torch": sum(ref) / sum(hip),
                                 "beats_torch_by_more_than_its_spread": beats(hip, ref)}
    return entry


def bench_step(shape, pca_loss, steps, warmup, dev):
    """The training step of tools/bench_tcga.py (same model, batch and optimiser) with the criterion as ``TrainCriterion``,
    under both settings of the switch, alternating over REPEATS repeats.  The shipped configs set ``pca_indep_loss`` only;
    ``pca_loss`` adds the feature term over pca_feature."""
    import bench_tcga as T
    from _util import make_args
    from mlgnn.graph import SharedTopology
    from mlgnn.optim import FlatAdam
    from models import get_model
    cfg, B = T.SHAPES[shape]
    NN, G, S, E = 5135 * 3, 25015, 438, 60000
    gen = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    args = make_args(**dict(cfg, pca_loss=pca_loss))
    model = get_model("multilevel_gnn")(args)
    mask = (torch.rand(G, generator=gen) > 0.3).float()
    model.set_pca_params(torch.randn(int(mask.sum()), args.pca_dim, generator=gen) * 0.1, mask)
    model.set_info_mask(mask[:, None].clone())
    seg = torch.sort(torch.randint(0, S, (G,), generator=gen))[0]
    model.set_pathway_indexs(seg.to(dev))
    model.to(dev).train()
    src, dst = torch.randint(0, NN, (E,), generator=gen), torch.randint(0, NN, (E,), generator=gen)
    ei = torch.cat([torch.stack([src, dst]) + b * NN for b in range(B)], dim=1).to(dev)
    match = torch.randint(0, NN, (G,), generator=gen)
    match[torch.rand(G, generator=gen) < 0.02] = -1
    w = torch.rand(E, 1, generator=gen) * 2 - 1
    batch = SimpleNamespace(x=torch.rand(B * NN, 1, device=dev), edge_index=ei, edge_attr=w.repeat(B, 1).to(dev),
                            gene_pca_match=match[None].repeat(B, 1).to(dev), raw_indice=seg[None].repeat(B, 1).to(dev),
                            age=torch.rand(B, device=dev))
    batch.shared_topology = SharedTopology(torch.stack([src, dst]).to(dev), w.to(dev), NN, B)
    y = torch.nn.functional.one_hot(torch.randint(0, 2, (B,), device=dev), 2).float()
    opt = FlatAdam(model, lr=5e-5, clip_grad_norm=20)
    crit = C.TrainCriterion("plain")

    def step():
        opt.bucket.release()
        pred, feat = model(batch)
        loss = crit(model, pred, feat, y)
        loss.backward()
        opt.bucket.collect()
        opt.step()
        return loss

    def run(count):
        for _ in range(count):
            step()

    out = {"shape": shape, "batch": B, "steps": steps, "pca_loss": bool(args.pca_loss), "fused": [], "torch": []}
    for _ in range(REPEATS):
        for leg, on in (("fused", True), ("torch", False)):
            with switched(C, "ENABLED", on):
                run(warmup)
                out[leg].append(wall(lambda: run(steps))[0] / steps)
    out["summary_ms_per_step"] = {"fused_mean": leg_summary(out["fused"])["mean"], "torch_mean": leg_summary(out["torch"])["mean"],
                                  "torch_spread": leg_summary(out["torch"])["spread"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=0, help="also time this many training steps per leg at the gbm and kirc shapes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "criterion.json"))
    a = ap.parse_args()
    need_gpu("bench_criterion.py")
    dev = torch.device("cuda:0")
    result = {"workload": "BCELoss (plain / per-sample weights) + pca feature loss, fp32: the op of csrc/criterion.hip "
                          "against the torch lines (MLGNN_CRITERION_FUSED=0), same tensors",
              "timing": "device events, mean of %d runs after %d warm-up runs, the two legs alternating over %d repeats, "
                        "one process" % (a.iters, a.warmup, REPEATS),
              "device": torch.cuda.get_device_name(0), "op": [], "step": []}
    bench_shape(*SHAPES[0], MODES[0], dev, a.warmup, a.iters)      # discarded: clocks, allocator and code objects settle
    for name, B, M in SHAPES:
        for mode in MODES:
            entry = bench_shape(name, B, M, mode, dev, a.warmup, a.iters)
            result["op"].append(entry)
            print(json.dumps(entry), flush=True)
    if a.steps:
        for shape in ("gbm", "kirc"):
            for pca_loss in (False, True):
                entry = bench_step(shape, pca_loss, a.steps, 3, dev)
                result["step"].append(entry)
                print(json.dumps(entry), flush=True)
    write_json(a.out, result)


if __name__ == "__main__":
    main()
