#!/usr/bin/env python3
"""``VectorQuantizer.forward`` of the VQ-VAE, fp32, on a latent ``[B, 438, D]`` against a codebook ``[K, D]`` at

  (B, D, K) = (64, 2, 512)      the default flags (final_channels = 1, pca_dim = 2)
              (64, 64, 512)     latent width 64 (final_channels = 32 of the shipped configs)
              (32, 64, 512)     the same at half the batch

Times, with device events (mean of 50 runs after 10 warm-up runs, one process), the method on the op
(``mlgnn.vector_quantize``, csrc/vq.hip) against the same method with the switch off (``MLGNN_VQ_FUSED=0``: the torch
lines, what the code before the op ran), forward and forward + backward, on the same latent, codebook and cotangents.
The two legs alternate over three repeats, so the torch leg's own spread is on record.  Also checks that both legs
agree on those inputs.  Writes profiles/vq_layer.json.  Development tool; run it under a time limit of its own
(``timeout -k 10 600 python tools/bench_vq.py``)."""
import argparse
import json
import os
import sys

import torch

from _bench import alternate, event_ms, leg_summary, need_gpu, switched, write_json

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multilevel-gnn_amd"))
from mlgnn import vq as V  # noqa: E402
from models.vae import VectorQuantizer  # noqa: E402

SHAPES = [(64, 2, 512), (64, 64, 512), (32, 64, 512)]
P = 438
REPEATS = 3


def bench_shape(shape, dev, warmup, iters):
    B, D, K = shape
    torch.manual_seed(1)
    layer = VectorQuantizer(K, D, 0.25).to(dev)
    z = torch.randn(B, P, D, device=dev).requires_grad_()
    g_out = torch.randn(B, P, D, device=dev)
    g_loss = torch.tensor(1.0, device=dev)
    w = layer.embedding.weight

    def forward():
        return layer(z)

    def step():
        z.grad = w.grad = None
        q, loss = forward()
        torch.autograd.backward([q, loss], [g_out, g_loss])

    res = {}
    for on in (True, False):
        with switched(V, "ENABLED", on):
            step()
            q, loss = forward()
        res[on] = (q.detach(), float(loss.detach()), z.grad.clone(), w.grad.clone())
    N = B * P
    entry = {"B": B, "P": P, "D": D, "K": K, "rows": N,
             "mflop_forward": 3 * N * K * D / 1e6,                  # subtract, multiply, add per (row, code, column)
             "mbytes_distance_matrix_gone": N * K * 4 / 1e6,
             "mbytes_forward": (2 * N * D + K * D + N) * 4 / 1e6,   # z in, out and index out, the codebook once
             "mbytes_index_scans_backward": K * N * 4 / 1e6,        # the by-code pass, out of L2
             "agreement": {"rows_with_another_code": int((res[True][0] != res[False][0]).any(-1).sum()),
                           "vq_loss_hip": res[True][1], "vq_loss_torch": res[False][1],
                           "grad_z_max_abs_diff_over_max_abs":
                               float((res[True][2] - res[False][2]).abs().max() / res[False][2].abs().max()),
                           "grad_codebook_max_abs_diff_over_max_abs":
                               float((res[True][3] - res[False][3]).abs().max() / res[False][3].abs().max())}}
    entry.update(alternate(REPEATS, {"hip": True, "torch": False},           # the legs alternate
                           {"forward_ms": lambda on: event_ms(forward, warmup, iters),
                            "forward_backward_ms": lambda on: event_ms(step, warmup, iters)},
                           entering=lambda on: switched(V, "ENABLED", on)))
    entry["summary"] = {}
    for key in ("forward_ms", "forward_backward_ms"):
        hip, ref = entry["hip"][key], entry["torch"][key]
        h, r = leg_summary(hip), leg_summary(ref)
        entry["summary"][key] = {"hip_mean": h["mean"], "torch_mean": r["mean"], "torch_spread": r["spread"],
                                 "hip_spread": h["spread"], "speedup_over_torch": sum(ref) / sum(hip)}
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vq_layer.json"))
    a = ap.parse_args()
    need_gpu("bench_vq.py")
    dev = torch.device("cuda:0")
    result = {"workload": "VectorQuantizer.forward of the VQ-VAE, fp32: the op of csrc/vq.hip against the torch lines "
                          "(MLGNN_VQ_FUSED=0), same latent, codebook and cotangents",
              "timing": "device events, mean of %d runs after %d warm-up runs, the two legs alternating over %d repeats, "
                        "one process" % (a.iters, a.warmup, REPEATS),
              "device": torch.cuda.get_device_name(0), "op": []}
    for shape in SHAPES:
        entry = bench_shape(shape, dev, a.warmup, a.iters)
        result["op"].append(entry)
        print(json.dumps(entry), flush=True)
    write_json(a.out, result)


if __name__ == "__main__":
    main()
