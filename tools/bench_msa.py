#!/usr/bin/env python3
"""The pathway self-attention readout (pathway_readout='MSA') at the workload's shape: B = 64 graphs x P = 146 pathway
tokens, 8 heads, d in {64, 128, 256}, fp32.

Times, with device events (mean of 50 runs after 10 warm-up runs, one process):
  (a) the attention op alone, forward and forward + backward, through the HIP kernels (csrc/mha.hip) and as torch ops
      (reshape, permute, two batched products, softmax) on the same qkv;
  (b) the whole layer, models.deepergcn.MSAReadout against a stock nn.TransformerEncoderLayer with the same weights, both
      in training mode with dropout 0.
Writes profiles/msa_readout.json.  Development tool; run it under a time limit of its own
(``timeout -k 10 300 python tools/bench_msa.py``)."""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

from _bench import event_ms, need_gpu, write_json

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multilevel-gnn_amd"))
from mlgnn import mha_attention  # noqa: E402
from models.deepergcn import MSAReadout, torch_attention  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=64)
    ap.add_argument("--tokens", type=int, default=146)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--widths", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--op-only", action="store_true", help="the HIP attention op alone (per-kernel profiles)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msa_readout.json"))
    a = ap.parse_args()
    need_gpu("bench_msa.py")
    dev = torch.device("cuda:0")
    B, P, H = a.graphs, a.tokens, a.heads
    result = {"workload": "%d graphs x %d tokens, %d heads, fp32, dim_feedforward 2048, dropout 0, training mode" % (B, P, H),
              "timing": "device events, mean of %d runs after %d warm-up runs" % (a.iters, a.warmup), "widths": []}
    for d in a.widths:
        torch.manual_seed(1)
        qkv = torch.randn(B * P, 3 * d, device=dev, requires_grad=True)
        cot = torch.randn(B * P, d, device=dev)
        x = torch.randn(B, P, d, device=dev, requires_grad=True)
        cot3 = cot.reshape(B, P, d)

        def op_step(op):
            qkv.grad = None
            torch.autograd.backward(op(qkv, B, H), cot)

        entry = {"d": d, "head_width": d // H}
        ops = (("hip", mha_attention),) if a.op_only else (("hip", mha_attention), ("torch_ops", torch_attention))
        for name, op in ops:
            entry["attention_" + name] = {"forward_ms": event_ms(lambda: op(qkv, B, H), a.warmup, a.iters),
                                          "forward_backward_ms": event_ms(lambda: op_step(op), a.warmup, a.iters)}
        if not a.op_only:
            ours = MSAReadout(d, H, batch_first=True, dropout=0.0).to(dev).train()
            stock = nn.TransformerEncoderLayer(d, H, batch_first=True, dropout=0.0).to(dev).train()
            stock.load_state_dict(ours.state_dict(), strict=True)

            def layer_step(layer):
                for p in list(layer.parameters()) + [x]:
                    p.grad = None
                torch.autograd.backward(layer(x), cot3)

            for name, layer in (("msa_readout", ours), ("stock_layer", stock)):
                entry["layer_" + name] = {"forward_ms": event_ms(lambda: layer(x), a.warmup, a.iters),
                                          "forward_backward_ms": event_ms(lambda: layer_step(layer), a.warmup, a.iters)}
            entry["attention_speedup_over_torch_ops"] = {k: entry["attention_torch_ops"][k] / entry["attention_hip"][k]
                                                         for k in entry["attention_hip"]}
            entry["layer_speedup_over_stock"] = {k: entry["layer_stock_layer"][k] / entry["layer_msa_readout"][k]
                                                 for k in entry["layer_msa_readout"]}
        result["widths"].append(entry)
        print(json.dumps(entry), flush=True)
    write_json(a.out, result)


if __name__ == "__main__":
    main()
