#!/usr/bin/env python3
"""The PathwayConv layer at the shape of the shipped cohort: B = 64 graphs x (5 135 gene + 146 pathway nodes), 8 338
membership edges per graph (25 015 / 3), d = 128 and d = 64, aggregators ``max`` and ``softmax``.

Two legs in ONE process on the same ``x`` and cotangent: the layer on the kernels (csrc/pathway_conv.hip, the MLP on the
destination rows only) and the same layer with ``MLGNN_PATHWAY_CONV`` off (index_select, the outer-product GEMM,
scatter_reduce / the softmax steps, the MLP on all rows).  Device-event means over ``--iters`` runs after ``--warmup``
runs, forward and forward + backward; the legs alternate over ``--repeats`` repeats, so each leg's own spread is on
record.  The op alone is timed too: its gathered bytes (E_p * 2d * 4, counted from the shapes) over its forward time is
the achieved gather rate -- NOT an HBM rate: a gene belongs to several pathways, so the distinct rows of Y that are read
(at most N * 2d * 4 bytes) are fewer than the gathered ones and repeats are served from cache.  Writes
profiles/pathway_conv.json.  Development tool."""
import argparse
import json
import os
import sys

import torch

from _bench import alternate, beats, event_ms, leg_summary, need_gpu, switched, write_json

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multilevel-gnn_amd"))
from mlgnn import pathway_conv as pc  # noqa: E402
from mlgnn.dense import linear  # noqa: E402
from models.gcn_lib.sparse.torch_vertex import PathwayConv  # noqa: E402


def spread(values):
    s = leg_summary(values)
    return {"mean_ms": s["mean"], "min_ms": s["min"], "max_ms": s["max"], "runs_ms": values}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=64)
    ap.add_argument("--genes", type=int, default=5135)
    ap.add_argument("--pathways", type=int, default=146)
    ap.add_argument("--members", type=int, default=8338)
    ap.add_argument("--widths", type=int, nargs="+", default=[128, 64])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pathway_conv.json"))
    a = ap.parse_args()
    need_gpu("bench_pathway_conv.py")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(2025)
    B, n = a.graphs, a.genes + a.pathways
    N, E = B * n, B * a.members
    seg = torch.sort(torch.randint(0, a.pathways, (a.members,), generator=gen))[0]
    src = torch.randint(0, a.genes, (a.members,), generator=gen)
    ei = torch.cat([torch.stack([src, a.genes + seg]) + g * n for g in range(B)], dim=1).to(dev)
    attr = (torch.rand(E, 2, generator=gen) * 2 - 1).to(dev)
    topo = pc.PathwayTopology(ei, attr, N)
    R = int(topo.rows.numel())
    result = {"workload": "%d graphs x (%d gene + %d pathway nodes), %d membership edges per graph: N = %d, E_p = %d, "
                          "R = %d destination rows" % (B, a.genes, a.pathways, a.members, N, E, R),
              "warmup": a.warmup, "iters": a.iters, "repeats": a.repeats,
              "note": "op_forward_gather_bytes_per_s counts every gathered row (E_p * 2d * 4 bytes); repeats of a source row "
                      "come from cache, so it is not an HBM rate", "cases": []}
    for d in a.widths:
        for aggr in ("max", "softmax"):
            torch.manual_seed(1)
            layer = PathwayConv(d, d, aggr=aggr, norm="layer", mlp_layers=2).to(dev)
            x = torch.randn(N, d, generator=gen).to(dev).requires_grad_(True)
            cot = torch.randn(N, d, generator=gen).to(dev)
            W, b = layer.msg_encoder.weight, layer.msg_encoder.bias

            def layer_fwd():
                return layer(x, topo if pc.PATHWAY_CONV else ei, attr, mask=True, residual=x)

            def layer_step():
                for p in list(layer.parameters()) + [x]:
                    p.grad = None
                torch.autograd.backward(layer_fwd(), cot)

            outs = {}

            def forward_backward_ms(flag):
                ms = event_ms(layer_step, a.warmup, a.iters)
                outs[flag] = layer_fwd().detach()                   # untimed, for the agreement of the legs
                return ms

            legs = alternate(a.repeats, {"kernels": True, "torch_ops": False},
                             {"forward": lambda flag: event_ms(layer_fwd, a.warmup, a.iters),
                              "forward_backward": forward_backward_ms},
                             entering=lambda flag: switched(pc, "PATHWAY_CONV", flag))
            y = linear(x.detach(), torch.cat([W[:, 0::2], W[:, 1::2]], dim=0)).detach().requires_grad_(True)
            rcot = torch.randn(R, d, device=dev)

            def op_fwd():
                return pc.pathway_aggregate(y, b, topo, aggr=aggr, t=1.0)

            def op_step():
                y.grad = None
                torch.autograd.backward(op_fwd(), rcot)

            op_f, op_fb = event_ms(op_fwd, a.warmup, a.iters), event_ms(op_step, a.warmup, a.iters)
            gather = E * 2 * d * 4
            entry = {"d": d, "aggr": aggr,
                     "legs": {k: {m: spread(v) for m, v in leg.items()} for k, leg in legs.items()},
                     "max_abs_difference_of_the_legs": float((outs[True] - outs[False]).abs().max()),
                     "op_forward_ms": op_f, "op_forward_backward_ms": op_fb, "op_gather_bytes": gather,
                     "op_distinct_source_rows_bytes": int(torch.unique(ei[0]).numel()) * 2 * d * 4,
                     "op_forward_gather_bytes_per_s": gather / (op_f * 1e-3)}
            k, t = entry["legs"]["kernels"], entry["legs"]["torch_ops"]
            entry["speedup_over_torch_ops"] = {m: t[m]["mean_ms"] / k[m]["mean_ms"] for m in k}
            # the switch's rule: forward + backward beats the torch leg by more than that leg's own spread
            entry["kernels_win_beyond_the_torch_spread"] = beats(legs["kernels"]["forward_backward"],
                                                                 legs["torch_ops"]["forward_backward"])
            result["cases"].append(entry)
            print(json.dumps(entry), flush=True)
    write_json(a.out, result)


if __name__ == "__main__":
    main()
