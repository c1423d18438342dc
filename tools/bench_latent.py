#!/usr/bin/env python3
"""The latent head of the VAE behind the projection pooling -- the tail of ``VAE.encoder`` (``enc_mu``,
``exp(enc_log_sigma)``, the batch-std and correlation losses, ``cat``) plus the KL term of ``VAE.vae_loss`` -- fp32, on a
pooled latent ``[B, 438, H]`` at

  (B, H) = (64, 2)       the default flags (final_channels = 1, pca_dim = 2)
           (64, 64)      latent width 64 (final_channels = 32 of the shipped configs)
           (32, 64)      the same at half the batch
           (64, 128)     the kernels' B * H limit

Times, with device events (mean of 50 runs after 10 warm-up runs, one process), ``VAE.encoder`` on a given pooled tensor
with the switch on (``mlgnn.vae_latent``, csrc/vae_latent.hip) against the same method with the switch off
(``MLGNN_VAE_LATENT_FUSED=0``: the torch lines, what the code before the op ran), forward and forward + backward, on the
same latent, parameters and cotangents.  The two legs alternate over three repeats, so the torch leg's own spread is on
record.  Also checks that both legs agree on those inputs.  Writes profiles/vae_latent.json.  Development tool; run it
under a time limit of its own (``timeout -k 10 600 python tools/bench_latent.py``)."""
import argparse
import json
import os
import sys

import torch

from _bench import alternate, event_ms, leg_summary, need_gpu, switched, write_json

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multilevel-gnn_amd"))
from mlgnn import latent as L  # noqa: E402
from models.vae import VAE  # noqa: E402

SHAPES = [(64, 2), (64, 64), (32, 64), (64, 128)]
P = 438
REPEATS = 3


class Head(torch.nn.Module):
    """``VAE.encoder`` and the KL lines of ``VAE.vae_loss`` on a given pooled tensor (the kernel front is not timed)."""
    encoder = VAE.encoder
    _mean_abs_offdiag_corr = staticmethod(VAE._mean_abs_offdiag_corr)

    def __init__(self, H):
        super().__init__()
        self.enc_mu = torch.nn.Linear(H, H)
        self.enc_log_sigma = torch.nn.Linear(H, H)
        with torch.no_grad():
            self.enc_log_sigma.weight.mul_(0.3)

    def _project(self, pooled):
        return pooled, None

    def forward(self, pooled):
        q_z, h, losses, _ = self.encoder(pooled)
        kld_sum = getattr(q_z, "kld_sum", None)                    # the lines of VAE.vae_loss
        if kld_sum is not None:
            kld = kld_sum.sum() / (q_z.loc.shape[0] * q_z.loc.shape[1])
        else:
            kld = torch.distributions.kl_divergence(q_z, torch.distributions.Normal(0, 1.)).sum(-1).mean()
        return h, losses[0], losses[2], kld


def bench_shape(shape, dev, warmup, iters):
    B, H = shape
    torch.manual_seed(1)
    head = Head(H).to(dev)
    pooled = torch.randn(B, 1, P, H, device=dev).requires_grad_()     # [B, C = 1, 438, k = H]: encoder flattens it to [B, 438, H]
    g_h = torch.randn(B, P, 2 * H, device=dev)
    g_one = [torch.tensor(v, device=dev) for v in (1.0, 1.0, 0.1)]
    params = list(head.parameters())

    def forward():
        return head(pooled)

    def step():
        pooled.grad = None
        for p in params:
            p.grad = None
        torch.autograd.backward(list(forward()), [g_h] + g_one)

    res = {}
    for on in (True, False):
        with switched(L, "ENABLED", on):
            before = dict(L.LATENT_STATS)
            step()
            took = "hip" if on else "torch"
            assert L.LATENT_STATS[took] == before[took] + 1, "the %s leg did not run" % took
            out = [t.detach() for t in forward()]
        res[on] = (out, [pooled.grad.clone()] + [p.grad.clone() for p in params])
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
    entry = {"B": B, "P": P, "H": H,
             "mbytes_forward": (3 * B * P * H + 2 * H * H + 2 * H + 3 * P) * 4 / 1e6,    # x in, mu and sigma out
             "mbytes_backward_partials": P * (2 * H * H + 2 * H) * 4 / 1e6,             # written once, read once
             "agreement": {"embedding": rel(res[True][0][0], res[False][0][0]),
                           "loss_std_hip": float(res[True][0][1]), "loss_std_torch": float(res[False][0][1]),
                           "loss_corr_hip": float(res[True][0][2]), "loss_corr_torch": float(res[False][0][2]),
                           "kld_hip": float(res[True][0][3]), "kld_torch": float(res[False][0][3]),
                           "grad_max_abs_diff_over_max_abs": [rel(a, b) for a, b in zip(res[True][1], res[False][1])]}}
    entry.update(alternate(REPEATS, {"hip": True, "torch": False},           # the legs alternate
                           {"forward_ms": lambda on: event_ms(forward, warmup, iters),
                            "forward_backward_ms": lambda on: event_ms(step, warmup, iters)},
                           entering=lambda on: switched(L, "ENABLED", on)))
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vae_latent.json"))
    a = ap.parse_args()
    need_gpu("bench_latent.py")
    dev = torch.device("cuda:0")
    result = {"workload": "the tail of VAE.encoder plus the KL term of VAE.vae_loss, fp32: the op of csrc/vae_latent.hip "
                          "against the torch lines (MLGNN_VAE_LATENT_FUSED=0), same latent, parameters and cotangents",
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
