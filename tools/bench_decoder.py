#!/usr/bin/env python3
"""The per-pathway decoders of the pre-training models (``foreach_decoder`` of models/vae.py), fp32, at the TCGA shape
``tools/bench_tcga.py`` uses -- 25 015 decoded genes in 438 segments drawn with seed 0 --:

  B   (final_channels, pca_dim)   decoder
  64  (1, 2)                      foreach_diffhidden
  32  (1, 2)                      foreach_diffhidden
  64  (32, 2)                     foreach_diffhidden
  64  (1, 2)                      foreach, decoder_dim = 64
  64  (1, 2)                      foreach, decoder_dim = 256

Times, with device events (mean of 50 runs after 10 warm-up runs, one process), the model's ``foreach_decoder`` on the
kernels of csrc/pathway_decoder.hip against the same method with the switch off (``MLGNN_DECODER_FUSED=0``: the block
loop for ``foreach_diffhidden``, the gathered row-dot for ``foreach``), forward and forward + backward, on the same
latent and cotangent.  The four ``torch.cat`` calls that pack the parameters (and their backward) are part of the op's
leg and are also timed alone.  The whole measurement is repeated (``--repeats``) so that the spread between repeats of
the replaced path is on record next to the comparison.  Also checks that both legs agree.  Writes
profiles/pathway_decoder.json.  Development tool; run it under a time limit of its own
(``timeout -k 10 900 python tools/bench_decoder.py``)."""
import argparse
import json
import os
import sys

import torch

from _bench import alternate, event_ms, leg_summary, need_gpu, switched, write_json

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multilevel-gnn_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _util import make_args  # noqa: E402
from mlgnn import decoder as D  # noqa: E402
from models import get_model  # noqa: E402

G, S = 25015, 438
CASES = [(64, 1, 2, "foreach_diffhidden", 4096), (32, 1, 2, "foreach_diffhidden", 4096),
         (64, 32, 2, "foreach_diffhidden", 4096), (64, 1, 2, "foreach", 64), (64, 1, 2, "foreach", 256)]
BASE = dict(model="vae", num_layers=2, hidden_channels=16, final_head=1, node_embedding=True, node_embedding_dim=16,
            gnn_name="sage", head_dim=8, conv_channel_list=[8, 8], conv_kernel_list=[1, 1], reorder_type="pca",
            channel_one=True, pathway_pool_dim=2, pathway_num=146)


def segments():
    """The segment of each decoded gene, as tools/bench_tcga.py draws it (its mask draw comes first)."""
    gen = torch.Generator().manual_seed(0)
    torch.rand(G, generator=gen)
    return torch.sort(torch.randint(0, S, (G,), generator=gen))[0]


def bench_case(case, seg, dev, warmup, iters, repeats):
    B, C, k, decoder_type, decoder_dim = case
    torch.manual_seed(1)
    model = get_model("vae")(make_args(**dict(BASE, final_channels=C, pca_dim=k, decoder_type=decoder_type,
                                              decoder_dim=decoder_dim)), None, seg).to(dev)
    blocks = list(model.decoder)
    params = [p for b in blocks for p in b.parameters()]
    H = C * k
    z = torch.randn(B, S, H, device=dev).requires_grad_()
    cot = torch.randn(B, G, device=dev)
    max_hid, max_out, total = model._dec_limits
    assert total == G and D.decoder_supported(z, max_hid, max_out, total), "the op does not take this case"

    def fwd():
        return model.foreach_decoder(z)

    def step():
        z.grad = None
        for p in params:
            p.grad = None
        (fwd() * cot).sum().backward()

    def pack():
        return [torch.cat([b[0].weight.reshape(-1) for b in blocks]), torch.cat([b[0].bias for b in blocks]),
                torch.cat([b[2].weight.reshape(-1) for b in blocks]), torch.cat([b[2].bias for b in blocks])]

    def pack_step():
        for p in params:
            p.grad = None
        sum(t.sum() for t in pack()).backward()

    hid = [b[0].out_features for b in blocks]
    n = [b[2].out_features for b in blocks]
    weights = sum(h * H + h + h * m + m for h, m in zip(hid, n))
    entry = {"B": B, "final_channels": C, "pca_dim": k, "H": H, "decoder_type": decoder_type,
             "decoder_dim": decoder_dim if decoder_type == "foreach" else None, "max_hid": max_hid, "max_out": max_out,
             "mflop_forward": 2 * B * sum(h * H + h * m for h, m in zip(hid, n)) / 1e6,
             "mbytes_weights": weights * 4 / 1e6, "mbytes_forward": (weights + B * S * H + B * G) * 4 / 1e6,
             "launches_op": {"forward": 1, "backward": 1, "packing_cats": 4}}
    stats = dict(D.DECODER_STATS)
    outs, grads = {}, {}
    for on in (True, False):
        with switched(D, "ENABLED", on):
            outs[on] = fwd().detach()
            step()
        grads[on] = [z.grad.clone()] + [p.grad.clone() for p in params]
    assert D.DECODER_STATS["hip"] == stats["hip"] + 2 and D.DECODER_STATS["torch"] == stats["torch"] + 2
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
    entry["agreement"] = {"out_max_abs_diff_over_max_abs": rel(outs[True], outs[False]),
                          "worst_grad_max_abs_diff_over_max_abs": max(rel(a, b) for a, b in zip(grads[True], grads[False]))}
    # the legs alternate inside every repeat; (the switch's setting, forward, forward + backward) of each
    runs = alternate(repeats, {"hip": (True, fwd, step), "torch": (False, fwd, step), "packing": (False, pack, pack_step)},
                     {"forward_ms": lambda leg: event_ms(leg[1], warmup, iters),
                      "forward_backward_ms": lambda leg: event_ms(leg[2], warmup, iters)},
                     entering=lambda leg: switched(D, "ENABLED", leg[0]))
    for name, rs in runs.items():
        entry[name] = {key: {stat: leg_summary(ms)[stat] for stat in ("mean", "min", "max")} for key, ms in rs.items()}
    # the claim: forward + backward through the op is not slower than the replaced path, within that path's own spread
    t = leg_summary(runs["torch"]["forward_backward_ms"])
    entry["speedup_over_torch"] = {key: entry["torch"][key]["mean"] / entry["hip"][key]["mean"] for key in entry["hip"]}
    entry["not_slower_forward_backward"] = entry["hip"]["forward_backward_ms"]["mean"] <= t["mean"] + t["spread"]
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", type=int, nargs="*", help="indices into the case table (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pathway_decoder.json"))
    a = ap.parse_args()
    need_gpu("bench_decoder.py")
    dev = torch.device("cuda:0")
    seg = segments()
    result = {"workload": "foreach_decoder of the pre-training models over 438 segments / 25 015 genes, fp32: one launch "
                          "per direction (plus the packing cats) against the same method with MLGNN_DECODER_FUSED=0",
              "timing": "device events, mean of %d runs after %d warm-up runs, %d alternating repeats, one process"
                        % (a.iters, a.warmup, a.repeats),
              "device": torch.cuda.get_device_name(0), "op": []}
    for i, case in enumerate(CASES):
        if a.cases and i not in a.cases:
            continue
        entry = bench_case(case, seg, dev, a.warmup, a.iters, a.repeats)
        result["op"].append(entry)
        print(json.dumps(entry), flush=True)
    write_json(a.out, result)


if __name__ == "__main__":
    main()
