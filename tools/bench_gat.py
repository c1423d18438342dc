#!/usr/bin/env python3
"""The graph-attention layer at the shipped-config shape (config/kirc.yaml with the reference's default gnn_name='gat'):
B = 64 samples x 15 405 nodes, 60 000 shared edges per sample, layers 32 -> 64 (8 heads) and 64 -> 32 (4 heads).

Times, with device events: the layer (Linear + attention + activation) forward and forward + backward, through the HIP
kernels (csrc/gat.hip) and with the attention replaced by its plain torch-op formulation on the same GPU; and the
attention op alone, whose kernel-side algorithmic bytes (counted below from the shapes) over its time give the share of
the 8 TB/s HBM peak.  Writes profiles/gat_layer.json.  Development tool."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

from _bench import event_ms, need_gpu, switched, write_json

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multilevel-gnn_amd"))
import mlgnn.gat  # noqa: E402
from mlgnn.graph import SharedTopology, sage_graph  # noqa: E402
from models.gcn_lib.sparse.torch_vertex import GraphConv  # noqa: E402

HBM_PEAK = 8.0e12
REAL_OP = mlgnn.gat.gat_aggregate


def torch_gat_aggregate(z, att_src, att_dst, bias, graph, heads, negative_slope=0.2, act_slope=1.0):
    """PyG's GATConv message passing in torch ops (gather, scatter-max, exp, two scatter-adds)."""
    n, d = z.shape
    H, C = heads, d // heads
    rp = graph.rowptr[:n + 1].long()
    dst = torch.repeat_interleave(torch.arange(n, device=z.device), rp[1:] - rp[:-1])
    src = graph.col[:dst.numel()].long()
    zz = z.reshape(n, H, C)
    a_s, a_d = (zz * att_src.reshape(1, H, C)).sum(-1), (zz * att_dst.reshape(1, H, C)).sum(-1)
    e = F.leaky_relu(a_s[src] + a_d[dst], negative_slope)
    idx = dst[:, None].expand(-1, H)
    mx = torch.full((n, H), float("-inf"), device=z.device).scatter_reduce(0, idx, e.detach(), "amax")
    p = torch.exp(e - mx[dst])
    s = torch.zeros((n, H), device=z.device).index_add(0, dst, p) + 1e-16
    alpha = p / s[dst]
    out = torch.zeros((n, H, C), device=z.device).index_add(0, dst, alpha[:, :, None] * zz[src]).reshape(n, d)
    if bias is not None:
        out = out + bias
    return out if act_slope == 1.0 else F.leaky_relu(out, act_slope)


def op_bytes(N, E, H, C):
    """Algorithmic bytes of the attention op's kernels (fp32 / int32): what each pass has to read and write once."""
    d = H * C
    scores = N * d * 4 + 2 * N * H * 4
    fwd = E * d * 4 + E * 4 + E * H * 4 + (N + 1) * 4 + N * H * 4 + N * d * 4 + N * H * 4 + N * 4
    pre = 2 * N * d * 4 + N * d * 4 + 2 * N * H * 4 + N * H * 16
    main = E * d * 4 + E * H * 16 + E * 8 + E * H * 4 + (N + 1) * 4 + 2 * N * d * 4 + 2 * N * H * 4
    finish = E * H * 4 + (N + 1) * 4 + 3 * N * d * 4 + N * H * 4
    return dict(forward=scores + fwd, backward=pre + main + finish)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=64)
    ap.add_argument("--nodes", type=int, default=15405)
    ap.add_argument("--edges", type=int, default=60000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--layer", type=int, default=None, help="0 or 1: that layer only (per-kernel profiles)")
    ap.add_argument("--no-torch-ops", action="store_true", help="skip the torch-op formulation (per-kernel profiles)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gat_layer.json"))
    a = ap.parse_args()
    need_gpu("bench_gat.py")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(2024)
    B, n = a.graphs, a.nodes
    N = B * n
    ei1 = torch.randint(0, n, (2, a.edges), generator=gen)
    ei = torch.cat([ei1 + b * n for b in range(B)], dim=1).to(dev)
    shared = SharedTopology(ei1, None, n, B).to(dev)
    graph, _ = sage_graph(ei, None, N, shared)
    E = int(graph.col.numel())
    result = {"workload": "%d graphs x %d nodes, %d shared edges per graph (+ one self loop per node): N = %d, E = %d"
                          % (B, n, a.edges, N, E), "hbm_peak_bytes_per_s": HBM_PEAK, "layers": []}
    shapes = ((32, 64, 8), (64, 32, 4))
    for cin, cout, heads in (shapes if a.layer is None else shapes[a.layer:a.layer + 1]):
        torch.manual_seed(1)
        layer = GraphConv(cin, cout, conv='gat', act='leakyrelu', heads=heads).to(dev)
        g = layer.gconv.gconv
        x = torch.randn(N, cin, device=dev, requires_grad=True)
        cot = torch.randn(N, cout, device=dev)
        z = torch.randn(N, cout, device=dev, requires_grad=True)

        def layer_fwd():
            return layer(x, ei, shared=shared)

        def layer_step():
            for p in list(layer.parameters()) + [x]:
                p.grad = None
            torch.autograd.backward(layer_fwd(), cot)

        def op_fwd():
            return mlgnn.gat.gat_aggregate(z, g.att_src, g.att_dst, g.bias, graph, heads, 0.2, 0.2)

        def op_step():
            for p in (z, g.att_src, g.att_dst, g.bias):
                p.grad = None
            torch.autograd.backward(op_fwd(), cot)

        entry = {"in": cin, "out": cout, "heads": heads, "algorithmic_bytes": op_bytes(N, E, heads, cout // heads)}
        for name, op in (("hip", REAL_OP), ("torch_ops", torch_gat_aggregate)):
            if name == "torch_ops" and a.no_torch_ops:
                continue
            with switched(mlgnn.gat, "gat_aggregate", op):
                entry[name] = {"layer_forward_ms": event_ms(layer_fwd, a.warmup, a.iters),
                               "layer_forward_backward_ms": event_ms(layer_step, a.warmup, a.iters),
                               "op_forward_ms": event_ms(op_fwd, a.warmup, a.iters),
                               "op_forward_backward_ms": event_ms(op_step, a.warmup, a.iters)}
        hip, ab = entry["hip"], entry["algorithmic_bytes"]
        bwd_ms = hip["op_forward_backward_ms"] - hip["op_forward_ms"]
        entry["hip_share_of_hbm_peak"] = {"op_forward": ab["forward"] / (hip["op_forward_ms"] * 1e-3) / HBM_PEAK,
                                          "op_backward": ab["backward"] / (bwd_ms * 1e-3) / HBM_PEAK}
        if "torch_ops" in entry:
            entry["speedup_over_torch_ops"] = {k: entry["torch_ops"][k] / hip[k] for k in hip}
        result["layers"].append(entry)
        print(json.dumps(entry), flush=True)
    write_json(a.out, result)


if __name__ == "__main__":
    main()
