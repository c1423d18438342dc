#!/usr/bin/env python3
"""Golden fixtures of the multi-omics model, from the reference's OWN classes (authoring container only):
``python tests/golden/make_golden_multiomix.py``.  The import stand-ins are those of ``make_golden.py`` (imported,
not changed); nothing in the test-suite imports this file.

* ``pathwayconv_{i}.npz``: ``PathwayConv`` alone (models/gcn_lib/sparse/torch_vertex.py:107-178), one per aggregator
  the reference can construct (max, softmax, softmax_sg, mean, add, softmax_sum) plus softmax with ``learn_t``:
  inputs, output, cotangent, all input and parameter gradients.
* ``multiomix_{i}.npz``: ``MultiOmixGCN`` (models/deepergcn_virtual_node.py): batch fields, ``pred``, cotangent,
  ``state_dict``, parameter gradients.

The reference offsets ``pathway_{omics}_edges`` in place on the batch: it is handed CLONES, the fixtures store the
unmutated tensors.  ``power`` / ``power_sum`` cannot be constructed in the reference (``TypeError``): no fixture."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

OMICS = ("mrna", "cnv", "mt")
GENES, PATHWAYS, MEMBERS = 40, 8, 60          # per graph: gene nodes, pathway nodes (the last rows), membership edges


def membership(gen, n_graphs, batched):
    """``(edges [B * MEMBERS, 2], attr [B * MEMBERS, 2])``: sources among the genes, destinations among the pathway rows
    (pathway 7 of every graph stays without an edge; duplicates included); ``batched``: global node ids."""
    n = GENES + PATHWAYS
    es = []
    for g in range(n_graphs):
        src = torch.randint(0, GENES, (MEMBERS,), generator=gen)
        dst = GENES + torch.randint(0, PATHWAYS - 1, (MEMBERS,), generator=gen)
        src[5:8], dst[5:8] = src[2:5], dst[2:5]
        es.append(torch.stack([src, dst], dim=1) + (g * n if batched else 0))
    attr = torch.randn(n_graphs * MEMBERS, 2, generator=gen)
    attr[::9, 1] = 0.0
    return torch.cat(es), attr


def compact_(model, ffn_units=16):
    """Keep the files small without changing what they pin: the reference's initial parameters are rounded to 10
    fractional bits (they compress); the parameters of ``pathway_gcns.0`` -- built, never called -- are zeroed; of the
    MSA layer's 2048 feed-forward units all but the first ``ffn_units`` are switched off (zero weights and bias: their
    gradients are zero too)."""
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.copy_(torch.round(p * 1024.0) / 1024.0)
            if ".pathway_gcns.0." in "." + name:
                p.zero_()
            if name.endswith("readout_func.linear1.weight") or name.endswith("readout_func.linear1.bias"):
                p[ffn_units:] = 0.0
            if name.endswith("readout_func.linear2.weight"):
                p[:, ffn_units:] = 0.0


def fx_pathwayconv(ref):
    gen = torch.Generator().manual_seed(1212)
    cfgs = [dict(d=16, aggr="max", norm="layer"),
            dict(d=16, aggr="softmax", t=1.0, norm="layer"),
            dict(d=32, aggr="softmax_sg", t=1.5, norm="layer"),
            dict(d=16, aggr="mean", norm="layer"),
            dict(d=16, aggr="add", norm="layer"),
            dict(d=16, aggr="softmax_sum", t=0.8, learn_t=True, y=0.3, learn_y=True, norm="layer"),
            dict(d=32, aggr="softmax", t=0.7, learn_t=True, msg_norm=True, learn_msg_scale=True, encode_edge=True,
                 edge_feat_dim=32, norm="layer")]
    for ci, cfg in enumerate(cfgs):
        cfg = dict(cfg)
        d = cfg.pop("d")
        B = 2
        N = B * (GENES + PATHWAYS)
        edges, attr = membership(gen, B, batched=True)
        ei = edges.t().contiguous()
        torch.manual_seed(1300 + ci)
        conv = ref.vertex.PathwayConv(d, d, mlp_layers=2, **cfg)
        conv.train()
        x = torch.randn(N, d, generator=gen, requires_grad=True)
        mask = torch.zeros(N, 1)
        mask[ei[1]] = 1.0
        out = conv(x, ei.clone(), attr.clone(), mask)
        c = MG.probe_weights(out, gen)
        named = {"x": x}
        named.update({"sd." + k: v for k, v in conv.named_parameters()})
        g = MG.grads_of((out * c).sum(), named)
        MG.save("pathwayconv_%d" % ci, cfg=np.array(repr(sorted(dict(cfg, d=d).items()))), x=x, edge_index=ei,
                edge_attr=attr, mask=mask, out=out, cot=c, sd=dict(conv.state_dict()), grad=g)


def fx_multiomix(ref):
    gen = torch.Generator().manual_seed(1313)
    base = dict(model="multiomix", num_layers=2, hidden_channels=16, dropout=0.0, conv_encode_edge=False,
                use_edge_attr=True, use_column="w", graph_pooling="mean", norm="layer", mlp_layers=2, block="res+",
                pathway_global_node=True, node_embedding=False, use_age=False, num_layer_head=1, pathway_num=PATHWAYS,
                pathway_readout=None, mul_attr=False, head_dropout=False)
    cases = [(dict(gcn_aggr="max", pathway_readout="maxpool", use_age=True, num_layer_head=2), 2, "eval"),
             (dict(gcn_aggr="softmax", learn_t=True, t=0.6, conv_encode_edge=True, msg_norm=True, learn_msg_scale=True), 3, "train"),
             (dict(gcn_aggr="mean", pathway_readout=None, graph_pooling="sum"), 2, "train"),
             (dict(gcn_aggr="softmax_sg", t=1.5, pathway_readout="MSA", hidden_channels=32, mlp_layers=1), 2, "eval"),
             (dict(gcn_aggr="softmax", norm="batch", pathway_readout=None), 3, "train"),
             (dict(gcn_aggr="max", block="plain", pathway_readout="maxpool", graph_pooling="max"), 2, "train"),
             (dict(gcn_aggr="add", pathway_readout=None, pathway_global_node=False), 2, "train"),
             (dict(gcn_aggr="softmax_sum", learn_t=True, t=0.8, y=0.25, learn_y=True, block="res+",
                   pathway_readout="maxpool", use_age=True), 2, "train")]
    n = GENES + PATHWAYS
    for ci, (over, B, mode) in enumerate(cases):
        a = MG.default_args(ref, **dict(base, **over))
        ei, ea, bvec = MG.small_graph(gen, B, n, 160, edge_dim=1)
        torch.manual_seed(1400 + ci)
        model = ref.multiomix.MultiOmixGCN(a)
        compact_(model)
        model.train() if mode == "train" else model.eval()      # dropout p = 0; 'eval' for BatchNorm1d / the MSA layer's dropout
        fields = dict(x=torch.randn(B * n, 3, generator=gen), edge_index=ei, edge_attr=ea, batch=bvec,
                      age=torch.rand(B, generator=gen), node_size=torch.tensor([n] * B))
        for o in OMICS:
            edges, attr = membership(gen, B, batched=False)
            fields["pathway_%s_edges" % o] = edges
            fields["pathway_%s_edges_num" % o] = torch.tensor([MEMBERS] * B)
            fields["pathway_%s_edge_attr" % o] = attr
            fields["pathway_%s_node_attr" % o] = torch.randn(B * PATHWAYS, 2, generator=gen)
        batch = SimpleNamespace(**{k: (v.clone() if k.endswith("_edges") else v) for k, v in fields.items()})
        out = model(batch)
        c = MG.probe_weights(out, gen)
        named = {"sd." + k: v for k, v in model.named_parameters()}
        names = [k for k, v in named.items() if v.requires_grad]
        gs = torch.autograd.grad((out * c).sum(), [named[k] for k in names], allow_unused=True)
        unused = np.array(sorted(k[3:] for k, g in zip(names, gs) if g is None))
        g = {k: (gr if gr is not None else torch.zeros_like(named[k])) for k, gr in zip(names, gs)}
        MG.save("multiomix_%d" % ci, over=np.array(repr(sorted(dict(base, **over).items()))), mode=np.array(mode),
                pred=out, cot=c, sd=dict(model.state_dict()), grad=g, unused=unused, **fields)


def main():
    ref = MG._reference()
    from models import deepergcn_virtual_node
    ref.multiomix = deepergcn_virtual_node
    torch.set_num_threads(4)
    MG.PACK_ABOVE = 40                      # (a zip member per tiny tensor costs more than the tensor)
    only = set(sys.argv[1:])
    for name, fx in [("pathwayconv", fx_pathwayconv), ("multiomix", fx_multiomix)]:
        if not only or name in only:
            fx(ref)


if __name__ == "__main__":
    main()
