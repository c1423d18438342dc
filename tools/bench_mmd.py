#!/usr/bin/env python3
"""The MMD term of the VAE pre-training loss over all pathways, fp32, at

  (B, P, H) = (32, 438, 64), (64, 438, 64)   latent width 64 (final_channels * pca_dim) at the two batch sizes
              (64, 438, 2)                   the default flags (final_channels = 1, pca_dim = 2)

for both kernel kinds ('imq', 'rbf').  Times, with device events (mean of 50 runs after 10 warm-up runs, one process),
the op ``mlgnn.mmd_per_pathway(...).mean()`` against the per-pathway loop it replaces (``VAE.compute_mmd`` once per
pathway -- what ``MLGNN_MMD_FUSED=0`` selects and what the code before the op ran), forward and forward + backward,
on the same ``z`` and the same prior.  Also checks that both legs agree on those inputs.  Writes profiles/mmd_loss.json.
Development tool; run it under a time limit of its own (``timeout -k 10 600 python tools/bench_mmd.py``)."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch

from _bench import event_ms, need_gpu, write_json

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multilevel-gnn_amd"))
from mlgnn import mmd as M  # noqa: E402
from models import get_model  # noqa: E402

SHAPES = [(32, 438, 64), (64, 438, 64), (64, 438, 2)]
KINDS = ["imq", "rbf"]
METHODS = ("compute_mmd", "compute_kernel", "compute_rbf", "compute_inv_mult_quad")


def bench_shape(shape, kind, dev, warmup, iters, z_var=2.0):
    B, P, H = shape
    torch.manual_seed(1)
    z = (0.3 * torch.randn(B, P, H, device=dev) + 0.5).requires_grad_()
    prior = torch.randn(B, P, H, device=dev)
    # the model's own methods, on an object that carries args and nothing else
    vae = type("ArgsCarrier", (), {m: getattr(get_model("vae"), m) for m in METHODS})()
    vae.args = SimpleNamespace(mmd_kernel_type=kind, z_var=z_var)

    def hip():
        return M.mmd_per_pathway(z, prior, kind, z_var).mean()

    def loop():
        return torch.stack([vae.compute_mmd(z[:, i, :], prior[:, i, :]) for i in range(P)]).mean()

    def step(fn):
        def run():
            z.grad = None
            fn().backward()
        return run

    a, b = hip(), loop()
    ga, gb = torch.autograd.grad(a, z)[0], torch.autograd.grad(b, z)[0]
    # pair distances, 3 multiply-adds per element and pair (T_pp, T_zz, T_pz); bytes the op has to move per direction
    entry = {"B": B, "P": P, "H": H, "kind": kind, "z_var": z_var,
             "mflop_forward": 2 * 3 * B * B * H * P / 1e6, "mbytes_forward": (2 * B * P * H + 4 * P) * 4 / 1e6,
             "mbytes_backward": (3 * B * P * H + P) * 4 / 1e6,
             "agreement": {"mmd_mean_hip": float(a), "mmd_mean_loop": float(b),
                           "grad_max_abs_diff_over_max_abs": float((ga - gb).abs().max() / gb.abs().max())}}
    for leg, fn in (("hip", hip), ("loop", loop)):
        entry[leg] = {"forward_ms": event_ms(fn, warmup, iters), "forward_backward_ms": event_ms(step(fn), warmup, iters)}
    entry["speedup_over_loop"] = {k: entry["loop"][k] / entry["hip"][k] for k in entry["hip"]}
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mmd_loss.json"))
    a = ap.parse_args()
    need_gpu("bench_mmd.py")
    dev = torch.device("cuda:0")
    result = {"workload": "MMD term of VAE.vae_loss over all pathways, fp32: one launch per direction against the "
                          "per-pathway loop (MLGNN_MMD_FUSED=0), same z and prior",
              "timing": "device events, mean of %d runs after %d warm-up runs, one process" % (a.iters, a.warmup),
              "device": torch.cuda.get_device_name(0), "op": []}
    for shape in SHAPES:
        for kind in KINDS:
            entry = bench_shape(shape, kind, dev, a.warmup, a.iters)
            result["op"].append(entry)
            print(json.dumps(entry), flush=True)
    write_json(a.out, result)


if __name__ == "__main__":
    main()
