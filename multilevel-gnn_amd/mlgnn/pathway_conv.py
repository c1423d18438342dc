"""PathwayConv's message + aggregation (the reference's models/gcn_lib/sparse/torch_vertex.py:107-178) over the
gene -> pathway-node membership edges, as ONE autograd node around the kernels of csrc/pathway_conv.hip.

Per edge ``j -> i`` with attributes ``a_e`` [2]::

    msg_e = msg_encoder(flatten(x_j (x) a_e)) = a_e0 * Y0[j] + a_e1 * Y1[j] + b,      Y_k = x W[:, k::2]^T

``Y = [Y0 | Y1]`` stays a separate GEMM node (:func:`mlgnn.dense.linear`); the op reduces the messages of every
destination row that has edges (``topology.rows``, ``R`` of ``N``) and returns ``[R, d]`` -- no ``[E, d]`` tensor exists.
``max`` and ``softmax`` run in the kernels; ``add`` and ``mean`` are, by linearity, two weighted sums of the existing
aggregation (:func:`pathway_linear_aggregate`).  fp32 only, no atomics (bitwise reproducible), no CPU path.

:class:`PathwayTopology` is what all layers of one forward pass (and forward + backward) share: the CSR both ways, the
compact row list, the attribute tables.  Building it costs ONE host synchronisation (for ``R``); a cache hit none."""
import os

import torch

from . import _lib
from .dense import _aligned
from .graph import CSRGraph, _same_view
from .ops import weighted_mean_aggregate

AGGR_MAX, AGGR_SOFTMAX = 2, 3
# (0: PathwayConv as torch lines -- index_select, the outer-product GEMM, scatter_reduce / the softmax steps; for A/B runs)
PATHWAY_CONV = os.environ.get("MLGNN_PATHWAY_CONV", "1") == "1"
STATS = _lib.stats("pathway_conv", suffix=" (MLGNN_PATHWAY_CONV=%d)" % PATHWAY_CONV, fwd=0, bwd=0, topology_build=0,
                   topology_hit=0, compact_layers=0, all_rows_layers=0, torch_layers=0)


class PathwayTopology:
    """Membership edges ``edge_index [2, E]`` (global node ids, ``src -> dst``) with attributes ``edge_attr [E, 2]`` over
    ``num_nodes`` nodes: ``graph`` (:class:`mlgnn.CSRGraph`), ``rows [R]`` int32 (the destinations that have edges,
    ascending), ``rows_long`` (the same as int64, for torch indexing), ``row_of [N]`` int32 (position in ``rows`` or -1),
    ``deg [R]`` (in-degree of ``rows``, fp32), ``attr_dst`` / ``attr_src [E, 2]`` (by-destination / by-source order)."""

    def __init__(self, edge_index, edge_attr, num_nodes):
        if edge_attr is None or edge_attr.dim() != 2 or edge_attr.shape[1] != 2 or edge_attr.shape[0] != edge_index.shape[1]:
            raise ValueError("pathway edge attributes must be [E, 2]")
        N = int(num_nodes)
        self.num_nodes, self.edge_index, self.edge_attr = N, edge_index, edge_attr
        self.graph = CSRGraph(edge_index, N)
        self.num_edges = self.graph.num_edges
        self.attr_dst, self.attr_src = self.graph.edge_table(edge_attr, 2)
        deg = self.graph.rowptr[1:N + 1] - self.graph.rowptr[:N]
        self.rows_long = torch.nonzero(deg > 0).reshape(-1)          # the ONE host synchronisation (R)
        self.rows = self.rows_long.to(torch.int32)
        R = int(self.rows.numel())
        self.row_of = torch.full((N,), -1, dtype=torch.int32, device=deg.device)
        self.row_of[self.rows_long] = torch.arange(R, dtype=torch.int32, device=deg.device)
        self.deg = deg[self.rows_long].to(torch.float32)
        STATS["topology_build"] += 1

    _CACHE = []          # [(key tensors, versions, num_nodes, topology)], most recent first
    CACHE_SIZE = 6       # three omics x (the batch in flight + the one before)

    @classmethod
    def from_cache(cls, key_tensors, num_nodes, build):
        """The topology ``build()`` made for these ``key_tensors`` (a tuple: the batch's membership tensors) the first
        time: a hit is the same tensors (or views of the same elements) at the same versions -- no device work, no
        synchronisation.  The entry holds the tensors, so their storage cannot be recycled under the cache."""
        N = int(num_nodes)
        vers = tuple(t._version for t in key_tensors)
        for k, ent in enumerate(cls._CACHE):
            if ent[2] == N and ent[1] == vers and len(ent[0]) == len(key_tensors) \
                    and all(_same_view(h, t) for h, t in zip(ent[0], key_tensors)):
                cls._CACHE.insert(0, cls._CACHE.pop(k))
                STATS["topology_hit"] += 1
                ent[3].graph._ordered_after_build()
                return ent[3]
        topo = build()
        cls._CACHE.insert(0, (tuple(key_tensors), vers, N, topo))
        del cls._CACHE[cls.CACHE_SIZE:]
        return topo

    @classmethod
    def clear_cache(cls):
        del cls._CACHE[:]


def pathway_conv_supported(y, topology=None):
    """fp32 device rows ``Y [N, 2d]`` with ``1 <= d <= 256`` and less than 4 GiB."""
    if not (torch.is_tensor(y) and y.is_cuda and y.dtype == torch.float32 and y.dim() == 2 and y.shape[1] % 2 == 0):
        return False
    E = topology.num_edges if topology is not None else 0
    return bool(_lib.lib.mlgnn_pathway_conv_supported(y.shape[0], E, y.shape[1] // 2))


class _PathwayAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, bias, t, topo, aggr_id, learn_t):
        y = _aligned(y)
        N, d = y.shape[0], y.shape[1] // 2
        R, E = int(topo.rows.numel()), topo.num_edges
        dev = y.device
        b = _aligned(bias.detach().reshape(-1).to(torch.float32)) if bias is not None else None
        t_dev = t.detach().reshape(-1).to(torch.float32) if torch.is_tensor(t) else None
        t_imm = 1.0 if t_dev is not None else float(t)
        out = torch.empty((R, d), dtype=torch.float32, device=dev)
        winner = torch.empty((R, d), dtype=torch.int32, device=dev) if aggr_id == AGGR_MAX else None
        lse = torch.empty((R, d), dtype=torch.float32, device=dev) if aggr_id == AGGR_SOFTMAX else None
        g = topo.graph
        _lib.call("mlgnn_pathway_conv_fwd", y, g.rowptr, g.col, topo.attr_dst, topo.rows, b, out, winner, lse, N, E, R,
                  d, aggr_id, t_imm, t_dev, _lib.stream())
        STATS["fwd"] += 1
        ctx.save_for_backward(y, b, t_dev, out, winner, lse)
        ctx.topo = topo
        ctx.cfg = (aggr_id, bool(learn_t), t_imm, bias.shape if bias is not None else None,
                   t.shape if torch.is_tensor(t) else None)
        return out

    @staticmethod
    def backward(ctx, go):
        y, b, t_dev, out, winner, lse = ctx.saved_tensors
        aggr_id, learn_t, t_imm, shape_b, shape_t = ctx.cfg
        topo, g = ctx.topo, ctx.topo.graph
        N, d = y.shape[0], y.shape[1] // 2
        R, E = int(topo.rows.numel()), topo.num_edges
        f32 = dict(dtype=torch.float32, device=y.device)
        need_b = ctx.needs_input_grad[1] and b is not None
        need_t = learn_t and ctx.needs_input_grad[2] and t_dev is not None
        go = _aligned(go.to(torch.float32))
        gy = torch.empty_like(y)
        gb = torch.empty(d, **f32) if need_b else None
        gt = torch.empty(1, **f32) if learn_t else None
        ws, floats = _lib.workspace("mlgnn_pathway_conv_bwd_workspace_floats", N, E, R, d, int(learn_t), device=y.device)
        _lib.call("mlgnn_pathway_conv_bwd", go, y, out, b, winner, lse, g.rowptr_t, g.col_t, g.pos_t, topo.attr_src,
                  topo.row_of, gy, gb, gt, ws, floats, N, E, R, d, aggr_id, t_imm, t_dev, int(learn_t), _lib.stream())
        STATS["bwd"] += 1
        return (gy, gb.reshape(shape_b) if need_b else None, gt.reshape(shape_t) if need_t else None, None, None, None)


def pathway_aggregate(y, bias, topology, aggr="max", t=1.0, learn_t=False):
    """``Y`` [N, 2d] (``Y0 | Y1`` side by side), ``bias`` [d] or None, ``topology`` a :class:`PathwayTopology` ->
    ``m[rows] + bias`` [R, d] for ``aggr`` in ``max`` / ``softmax`` (``t``: a float, or a one-element device tensor;
    ``learn_t``: the gradient also runs through the softmax weights and to ``t``)."""
    _lib.require_gpu(y, "mlgnn.pathway_conv")
    if aggr not in ("max", "softmax"):
        raise ValueError("pathway_aggregate: aggr must be 'max' or 'softmax' (add / mean: pathway_linear_aggregate)")
    if not pathway_conv_supported(y, topology):
        raise ValueError("pathway_aggregate: unsupported input %s %s (fp32 [N, 2d], 1 <= d <= 256, < 4 GiB)"
                         % (tuple(y.shape), y.dtype))
    if topology.num_nodes != y.shape[0] or not topology.rows.is_cuda:
        raise ValueError("pathway_aggregate: the topology must live on the device and have %d nodes" % y.shape[0])
    if bias is not None and bias.numel() != y.shape[1] // 2:
        raise ValueError("pathway_aggregate: bias must hold d = %d values" % (y.shape[1] // 2))
    if learn_t and aggr != "softmax":
        raise ValueError("pathway_aggregate: learn_t needs the softmax aggregator")
    if torch.is_tensor(t) and (t.numel() != 1 or not t.is_cuda):
        raise ValueError("pathway_aggregate: a tensor t must be one element on the device")
    if topology.rows.numel() == 0:
        return y.new_zeros((0, y.shape[1] // 2)) + 0.0 * y.sum()
    return _PathwayAggregate.apply(y, bias, t, topology, AGGR_MAX if aggr == "max" else AGGR_SOFTMAX, bool(learn_t))


def pathway_linear_aggregate(x, weight, bias, topology, mean=False):
    """``add`` / ``mean`` of the messages, [R, d]: by linearity ``sum_e msg_e = [S0 | S1][rows] [W0 | W1]^T + deg b`` with
    ``S_k = sum_e a_ek x_j`` -- two calls of the weighted CSR aggregation and one product on the destination rows."""
    _lib.require_gpu(x, "mlgnn.pathway_conv")
    a = topology.edge_attr
    s0 = weighted_mean_aggregate(x, topology.graph, a[:, 0], mean=mean)
    s1 = weighted_mean_aggregate(x, topology.graph, a[:, 1], mean=mean)
    rows = topology.rows_long
    s = torch.cat([s0.index_select(0, rows), s1.index_select(0, rows)], dim=1)
    out = s.matmul(torch.cat([weight[:, 0::2], weight[:, 1::2]], dim=1).t())
    if bias is not None:
        out = out + (bias if mean else topology.deg[:, None] * bias)
    return out
