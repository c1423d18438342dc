#!/usr/bin/env python3
"""The PathCNN baseline at the workload's shape: B = 64 patients, pca_dim = 2 (the 146 x 6 pathway image), fp32.

Times, with device events (mean of 50 runs after 10 warm-up runs, one process):
  (a) the convolution op alone, forward and forward + backward (input, weight and bias gradients, ReLU fused), at the
      model's three shapes 1 -> 32, 32 -> 64 and 64 -> 64 (k = 3);
  (b) the whole training step of ``get_model('pathcnn')`` with ``learnable_pca`` (projection of 25015 raw member values,
      convolutions, pool, head, BCE + feature loss, backward, fused Adam), as train_harness.py runs it.
Each once on the HIP path (csrc/conv2d.hip) and once on the convolution library -- what ``MLGNN_PATH_CONV=0`` selects;
here the switch ``mlgnn.conv.ENABLED`` is flipped inside one process so that both legs share the session.  The warm-up
runs come first, so the library's run-time solver search is not in the timed region.
Writes profiles/pathcnn.json.  Development tool; run it under a time limit of its own
(``timeout -k 10 300 python tools/bench_pathcnn.py``)."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch

from _bench import event_ms, need_gpu, switched, write_json

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multilevel-gnn_amd"))
from mlgnn import conv  # noqa: E402
from mlgnn.optim import FlatAdam  # noqa: E402
from models import get_model  # noqa: E402
import train_harness  # noqa: E402


def bench_op(B, H, W, cin, cout, k, dev, warmup, iters):
    torch.manual_seed(1)
    m = conv.PathConv2d(cin, cout, k, padding=k // 2).to(dev)
    x = torch.randn(B, H, W, cin, device=dev).permute(0, 3, 1, 2).requires_grad_()       # channel-last, as the model has it
    cot = torch.randn(B, H, W, cout, device=dev).permute(0, 3, 1, 2)

    def step():
        x.grad = m.weight.grad = m.bias.grad = None
        torch.autograd.backward(m(x, relu=True), cot)

    entry = {"cin": cin, "cout": cout, "k": k, "gflop_forward": 2e-9 * B * H * W * cin * cout * k * k}
    for name, on in (("hip", True), ("library", False)):
        with switched(conv, "ENABLED", on):
            entry[name] = {"forward_ms": event_ms(lambda: m(x, relu=True), warmup, iters),
                           "forward_backward_ms": event_ms(step, warmup, iters)}
    entry["speedup_over_library"] = {k_: entry["library"][k_] / entry["hip"][k_] for k_ in entry["hip"]}
    return entry


def bench_step(B, pca_dim, dev, warmup, iters, more_conv):
    G = 25015
    args = SimpleNamespace(**dict(train_harness.DEFAULTS, model="pathcnn", learnable_pca=True, pca_dim=pca_dim,
                                  more_conv=more_conv, pca_loss=True, pca_indep_loss=True))
    gen = torch.Generator().manual_seed(2)
    seg = torch.sort(torch.cat([torch.arange(438), torch.randint(0, 438, (G - 438,), generator=gen)]))[0]
    batch = SimpleNamespace(raw_data=torch.rand(B, G, generator=gen).to(dev), raw_indice=seg[None, :].expand(B, G).to(dev),
                            age=torch.rand(B, generator=gen).to(dev))
    target = torch.nn.functional.one_hot(torch.randint(0, 2, (B,), generator=gen), 2).float().to(dev)
    def train_step_ms():
        torch.manual_seed(3)
        model = get_model("pathcnn")(args)
        mask = torch.ones(G)
        model.set_pca_params(torch.randn(G, pca_dim) * 0.05, mask)
        model.set_info_mask(mask[:, None].clone())
        model.set_pathway_indexs((seg // 3).to(dev))
        model.to(dev).train()
        opt = FlatAdam(model, lr=1e-4)
        bucket = opt.bucket
        bce = torch.nn.BCELoss()

        def step():
            pred, feat = model(batch)
            floss = model.get_feature_loss(feat)
            bucket.release()
            (bce(pred, target) + floss).backward()
            bucket.collect()
            bucket.all_reduce_mean()
            opt.step()

        return event_ms(step, warmup, iters)

    entry = {"more_conv": more_conv}
    for name, on in (("hip", True), ("library", False)):
        with switched(conv, "ENABLED", on):
            entry[name] = {"train_step_ms": train_step_ms()}
    entry["speedup_over_library"] = entry["library"]["train_step_ms"] / entry["hip"]["train_step_ms"]
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patients", type=int, default=64)
    ap.add_argument("--pca_dim", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pathcnn.json"))
    a = ap.parse_args()
    need_gpu("bench_pathcnn.py")
    dev = torch.device("cuda:0")
    B, H, W = a.patients, 146, 3 * a.pca_dim
    result = {"workload": "PathCNN, %d patients x 146 x %d image, k = 3, fp32" % (B, W),
              "timing": "device events, mean of %d runs after %d warm-up runs; 'library' = the convolution library "
                        "(MLGNN_PATH_CONV=0), solver search in the warm-up" % (a.iters, a.warmup),
              "device": torch.cuda.get_device_name(0), "conv": [], "train_step": []}
    for cin, cout in ((1, 32), (32, 64), (64, 64)):
        entry = bench_op(B, H, W, cin, cout, 3, dev, a.warmup, a.iters)
        result["conv"].append(entry)
        print(json.dumps(entry), flush=True)
    for more_conv in (False, True):
        entry = bench_step(B, a.pca_dim, dev, a.warmup, a.iters, more_conv)
        result["train_step"].append(entry)
        print(json.dumps(entry), flush=True)
    write_json(a.out, result)


if __name__ == "__main__":
    main()
