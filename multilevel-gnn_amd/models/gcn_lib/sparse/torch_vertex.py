"""Sparse graph convolutions on the HIP CSR kernels (interface of the reference's
``models/gcn_lib/sparse/torch_vertex.py``: ``GENConv`` :12-104, ``SAGEConv`` :226-294,
``RSAGEConv`` :297-304, ``GATConv`` :207-223, ``GraphConv`` :338-363, ``PathwayConv`` :107-178).

Provided: ``gen``, ``sage``, ``rsage`` (the shipped configs), ``gat`` (the reference's default ``gnn_name``) and the
multi-omics model's ``PathwayConv`` (the membership step; ``MLGNN_PATHWAY_CONV=0``: its torch lines); the other
PyG-wrapper types (edge/mr/gcn/gin) raise ``NotImplementedError`` -- the reference's ``GraphConv.forward`` cannot call
them either.
"""
import math
import os

import torch
import torch.nn.functional as F
from torch import nn

from mlgnn import LowRankEdge, TableEdge, as_graph, weighted_mean_aggregate
from mlgnn import gat as mlgnn_gat
from mlgnn.dense import linear
from mlgnn.graph import sage_graph
from mlgnn.norm import msg_norm_add
from .torch_message import GenMessagePassing, MsgNorm, PathwayMessagePassing
from .torch_nn import MLP, act_layer, norm_layer

_SAGE_FUSED = os.environ.get("MLGNN_SAGE_FUSED", "1") == "1"      # (0: the separate aggregate / lin_r / cat / Linear / act ops, for A/B runs)


class GENConv(GenMessagePassing):
    """GENeralized graph convolution: ``MLP(x + [MsgNorm] aggregate(relu(x_j + e_ij) + eps))``."""

    def __init__(self, in_dim, emb_dim, aggr='softmax', t=1.0, learn_t=False, p=1.0, learn_p=False,
                 y=0.0, learn_y=False, gnn_encoder='linear', msg_norm=False, learn_msg_scale=True,
                 encode_edge=False, bond_encoder=False, edge_feat_dim=None, norm='batch', mlp_layers=2,
                 eps=1e-7, pca_only=False):
        super().__init__(aggr=aggr, t=t, learn_t=learn_t, p=p, learn_p=learn_p, y=y, learn_y=learn_y)
        if gnn_encoder != 'linear':
            raise NotImplementedError("gnn_encoder=%r is outside the accelerated path" % (gnn_encoder,))
        if bond_encoder:
            raise NotImplementedError("OGB bond encoder is outside the accelerated path")
        self.gnn_encoder = gnn_encoder
        self.feature_encoder = MLP([in_dim] + [in_dim * 2] * (mlp_layers - 1) + [emb_dim], norm=norm, last_lin=True)
        self.eps = eps
        self.encode_edge = encode_edge
        self.bond_encoder = bond_encoder
        self.msg_norm = MsgNorm(learn_msg_scale=learn_msg_scale) if msg_norm else None
        if encode_edge:
            self.edge_encoder = nn.Linear(edge_feat_dim, in_dim)
        self.pca_only = pca_only

    def forward(self, x, edge_index, edge_attr=None, residual=None, post_norm=None):
        """``edge_index``: COO ``[2, E]`` or a prebuilt :class:`mlgnn.CSRGraph`.
        ``residual``: added to the result inside the last Linear's epilogue (the caller's ``conv(...) + h``).
        ``post_norm = (nn.LayerNorm, relu)``: the caller's next step is ``relu?(norm(result))`` (the res+ block's
        pre-conv norm, deepergcn.py:236-241) -- returns ``(result, relu?(norm(result)))``, the second value written by
        the last Linear's epilogue instead of by a pass of its own.
        ``edge_attr``: ``[E, d_e]`` tensor, a :class:`mlgnn.LowRankEdge` (raw attributes kept factored
        through the Linear encoders: no ``[E, d]`` tensor, no edge GEMM) or a :class:`mlgnn.TableEdge`
        (one row of a small table per edge: the edge-type embedding)."""
        if self.pca_only:
            return self.feature_encoder(x)
        graph = as_graph(edge_index, x.shape[0])
        if isinstance(edge_attr, (LowRankEdge, TableEdge)):
            edge = edge_attr.through_linear(self.edge_encoder.weight, self.edge_encoder.bias) \
                if self.encode_edge else edge_attr
        elif edge_attr is not None:
            edge = self.edge_encoder(edge_attr) if self.encode_edge else edge_attr
            if edge.dim() != 2:                   # (a 2-D embedding is passed on as the object it is: it may carry the
                edge = edge.flatten(1)            #  shared-gradient tag of mlgnn.share_edge_gradient)
        else:
            edge = None
        flat = x.flatten(1)
        if self.msg_norm is None:
            h = self.reduce_messages(flat, graph, edge, self.eps, add_root=True)       # x + m in one pass
        else:
            h = msg_norm_add(flat, self.reduce_messages(flat, graph, edge, self.eps), self.msg_norm.msg_scale)
        if h.shape != x.shape:                    # (a same-shape reshape would drop the row-max tag of the kernel's output)
            h = h.reshape(x.shape)
        if isinstance(self.feature_encoder, MLP) and (residual is not None or post_norm is not None):
            return self.feature_encoder(h, residual=residual, post_norm=post_norm)
        out = self.feature_encoder(h)
        return out if residual is None else out + residual


class PathwayConv(PathwayMessagePassing):
    """Second message-passing step over the gene -> pathway-node membership edges (torch_vertex.py:107-178):
    ``relu(MLP(x + aggregate(msg_encoder(flatten(x_j (x) a_e))))) * mask``, ``a_e`` the edge's two attributes.

    ``msg_norm.msg_scale`` and ``edge_encoder`` exist for ``state_dict`` parity; the reference's forward uses neither.
    With ``mask=True`` (the destination mask: 1 exactly where a node has an incoming membership edge) only those ``R``
    rows are non-zero, and the MLP runs on them alone -- exact whenever the MLP's norm is per row.  A BatchNorm in
    training mode takes its statistics over all ``N`` rows in the reference: the layer then runs all rows."""

    def __init__(self, in_dim, emb_dim, aggr='softmax', t=1.0, learn_t=False, p=1.0, learn_p=False,
                 y=0.0, learn_y=False, msg_norm=False, learn_msg_scale=True, encode_edge=False, bond_encoder=False,
                 edge_feat_dim=None, norm='batch', mlp_layers=2, eps=1e-7):
        super().__init__(aggr=aggr, t=t, learn_t=learn_t, p=p, learn_p=learn_p, y=y, learn_y=learn_y)
        if bond_encoder:
            raise NotImplementedError("OGB bond encoder is outside the accelerated path")
        self.mlp = MLP([in_dim] + [in_dim * 2] * (mlp_layers - 1) + [emb_dim], norm=norm, last_lin=True)
        self.msg_encoder = nn.Linear(2 * in_dim, in_dim)
        self.eps = eps
        self.encode_edge = encode_edge
        self.bond_encoder = bond_encoder
        self.msg_norm = MsgNorm(learn_msg_scale=learn_msg_scale) if msg_norm else None
        if encode_edge:
            self.edge_encoder = nn.Linear(edge_feat_dim, in_dim)
        self.all_rows = False           # (True: the MLP over all N rows even where the compact form is exact; for A/B runs)

    def _batch_statistics(self):
        return self.training and any(isinstance(m, nn.modules.batchnorm._BatchNorm) for m in self.mlp)

    def forward(self, x, edge_index, edge_attr=None, mask=None, residual=None):
        """``edge_index``: COO ``[2, E_p]`` (global node ids) or a prebuilt :class:`mlgnn.pathway_conv.PathwayTopology`
        (then ``edge_attr`` may be omitted: the topology holds it).  ``mask``: None, a ``[N, 1]`` tensor, or True for
        the destination mask.  ``residual``: added to the result (the caller's ``conv(...) + h``)."""
        from mlgnn import pathway_conv as pc
        topo = edge_index if isinstance(edge_index, pc.PathwayTopology) else None
        if topo is not None and edge_attr is None:
            edge_attr = topo.edge_attr
        if edge_attr is None:
            raise ValueError("PathwayConv needs the [E, 2] edge attributes (its message encoder is Linear(2 * in_dim, in_dim))")
        W, b = self.msg_encoder.weight, self.msg_encoder.bias
        if not pc.PATHWAY_CONV:
            ei = topo.edge_index if topo is not None else edge_index
            pc.STATS["torch_layers"] += 1
            out = F.relu(self.mlp(x + self.reduce_pathway_messages_torch(x, ei, edge_attr, W, b)))
            if mask is True:
                mask = torch.zeros((x.shape[0], 1), dtype=x.dtype, device=x.device).index_fill_(0, ei[1], 1.0)
            if mask is not None:
                out = out * mask
            return out if residual is None else out + residual
        if topo is None:
            topo = pc.PathwayTopology.from_cache((edge_index, edge_attr), x.shape[0],
                                                 lambda: pc.PathwayTopology(edge_index, edge_attr, x.shape[0]))
        m = self.reduce_pathway_messages(x, topo, W, b)                          # [R, d]
        rows = topo.rows_long
        if mask is True and not self.all_rows and not self._batch_statistics():
            pc.STATS["compact_layers"] += 1
            out = F.relu(self.mlp(x.index_select(0, rows) + m))
            base = residual if residual is not None else torch.zeros_like(x)
            return base.index_add(0, rows, out)
        pc.STATS["all_rows_layers"] += 1
        out = F.relu(self.mlp(x.index_add(0, rows, m)))
        if mask is True:
            mask = (topo.row_of >= 0).to(out.dtype).unsqueeze(1)
        if mask is not None:
            out = out * mask
        return out if residual is None else out + residual


class Linear(nn.Module):
    """Bias-optional affine map that is deliberately NOT an ``nn.Linear`` subclass, like the PyG
    ``Linear`` the reference's SAGE base class creates: the models' xavier ``init_weight`` sweeps
    (multilevel_gnn.py:294-299) skip it, so it keeps kaiming-uniform(a=sqrt 5) initial values."""

    def __init__(self, in_channels, out_channels, bias=True):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if bias:
            bound = 1.0 / math.sqrt(in_channels)
            nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x):
        return F.linear(x, self.weight, self.bias)


class SAGEConv(nn.Module):
    """Weighted-mean GraphSAGE: ``nn(cat(x, mean_j((x_j * w_ij [- x_i]) W_r^T)))``.

    The reference multiplies every EDGE by ``W_r`` before the mean (torch_vertex.py:279-286);
    the mean is linear, so the kernel reduces ``x_j * w_ij`` first and ``W_r`` is applied to ``N``
    rows instead of ``E + N``.  ``lin_l`` exists only for ``state_dict`` compatibility (the
    reference never uses it either)."""

    def __init__(self, in_channels, out_channels, nn, norm=True, bias=True, relative=False, **kwargs):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.relative = relative
        self.lin_l = Linear(in_channels, out_channels, bias=bias)
        self.lin_r = Linear(in_channels, out_channels, bias=False)
        self.nn = nn
        self.normalize = norm
        if bias:
            self.bias = torch.nn.Parameter(torch.zeros(out_channels))
        else:
            self.bias = None

    def _fused_update(self):
        """``(slope,)`` when ``self.nn`` is the shipped ``Linear -> LeakyReLU / ReLU`` (or a bare Linear) and nothing else
        of this conv stands in the way of the one-product form (mlgnn.sage); None otherwise."""
        mods = list(self.nn) if isinstance(self.nn, nn.Sequential) else None
        if mods is None or self.normalize or self.bias is not None or not mods or type(mods[0]) is not nn.Linear:
            return None
        if len(mods) == 1:
            return (1.0,)
        if len(mods) == 2 and isinstance(mods[1], nn.LeakyReLU) and mods[1].negative_slope > 0:
            return (float(mods[1].negative_slope),)
        if len(mods) == 2 and type(mods[1]) is nn.ReLU:
            return (0.0,)
        return None

    def forward(self, x, edge_index, size=None, edge_attr=None, row_scale=None, shared=None):
        """``row_scale`` [N] or None: the caller's next step is ``out * row_scale[:, None]`` (MultilevelGNN's value mask,
        multilevel_gnn.py:205-207) -- applied here, in the update's epilogue when the fused layer runs.
        ``shared``: the batch's :class:`mlgnn.graph.SharedTopology` (every sample carries the same graph) or None."""
        if size is not None:
            raise NotImplementedError("bipartite propagation is outside the accelerated path")
        x = x.unsqueeze(-1) if x.dim() == 1 else x
        graph, weight = sage_graph(edge_index, edge_attr, x.shape[0], shared)
        fused = self._fused_update() if _SAGE_FUSED else None
        if fused is not None and (row_scale is None or not row_scale.requires_grad):
            from mlgnn.sage import sage_layer, sage_layer_supported
            lin = self.nn[0]
            if sage_layer_supported(x, lin.weight, self.lin_r.weight, False):
                return sage_layer(x, graph, weight, lin.weight, lin.bias, self.lin_r.weight, fused[0], self.relative,
                                  row_scale)
        out = self._forward_unfused(x, graph, weight)
        return out if row_scale is None else out * row_scale.reshape(-1, 1)

    def _forward_unfused(self, x, graph, weight):
        agg = weighted_mean_aggregate(x, graph, weight, mean=True)
        if self.relative:
            agg = agg - x                    # every node has its self loop: mean_j(x_i) = x_i
        aggr_out = linear(agg, self.lin_r.weight)          # tall-matrix weight gradient on the MFMA kernel
        if self.bias is not None:
            aggr_out = aggr_out + self.bias
        out = self.nn(torch.cat((x, aggr_out), dim=1))
        if self.normalize:
            out = F.normalize(out, p=2, dim=-1)
        return out


class RSAGEConv(SAGEConv):
    def __init__(self, in_channels, out_channels, act='relu', norm=False, mlp_norm=None, bias=True,
                 relative=False, drop=0.0):
        nn_ = MLP([out_channels + in_channels, out_channels], act, mlp_norm, bias, drop=drop)
        super().__init__(in_channels, out_channels, nn_, norm, False, relative)


class _PygGAT(nn.Module):
    """Parameters of PyG 2.2 ``GATConv(in, C, heads=H, bias=bias)`` under its attribute names: ``lin_src`` (bias-free, not
    an ``nn.Linear``: the models' xavier sweeps skip it) and ``lin_dst``, the SAME module (``state_dict`` lists both
    weights, ``parameters()`` yields one), ``att_src`` / ``att_dst`` [1, H, C], ``bias`` [H * C]; glorot / zeros."""

    def __init__(self, in_channels, out_channels, heads=1, bias=True, negative_slope=0.2):
        super().__init__()
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.negative_slope = negative_slope
        self.lin_src = Linear(in_channels, heads * out_channels, bias=False)
        self.lin_dst = self.lin_src
        self.att_src = nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_dst = nn.Parameter(torch.empty(1, heads, out_channels))
        self.bias = nn.Parameter(torch.zeros(heads * out_channels)) if bias else None
        for t in (self.lin_src.weight, self.att_src, self.att_dst):
            a = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))          # PyG's glorot
            nn.init.uniform_(t, -a, a)


class GATConv(nn.Module):
    """Graph attention: ``unlinear(softmax-weighted sum_j z_j + bias)``, ``z = lin_src(x)``, over the edges with the
    input's self loops replaced by one per node (the rewrite SAGEConv uses).  The projection is :func:`mlgnn.dense.linear`,
    everything per edge is :func:`mlgnn.gat.gat_aggregate`; a leading ReLU / LeakyReLU of ``unlinear`` runs in its
    epilogue.  ``out_channels`` is per head: the output is ``heads * out_channels`` wide; the norm of ``unlinear`` is built
    ``out_channels`` wide as the reference writes it (meaningful for one head only)."""

    def __init__(self, in_channels, out_channels, act='relu', norm=None, bias=True, heads=8):
        super().__init__()
        self.gconv = _PygGAT(in_channels, out_channels, heads, bias=bias)
        m = []
        if act:
            m.append(act_layer(act))
        if norm:
            m.append(norm_layer(norm, out_channels))
        self.unlinear = nn.Sequential(*m)

    def _epilogue(self):
        """``(slope of the activation the kernel applies, the modules of unlinear left to run)``"""
        mods = list(self.unlinear)
        if mods and type(mods[0]) is nn.ReLU:
            return 0.0, mods[1:]
        if mods and type(mods[0]) is nn.LeakyReLU and mods[0].negative_slope > 0:
            return float(mods[0].negative_slope), mods[1:]
        return 1.0, mods

    def forward(self, x, edge_index, edge_attr=None, row_scale=None, shared=None):
        """``edge_attr`` is ignored (the reference's wrapper drops it); ``row_scale`` / ``shared``: see SAGEConv."""
        x = x.unsqueeze(-1) if x.dim() == 1 else x
        graph, _ = sage_graph(edge_index, None, x.shape[0], shared)
        g = self.gconv
        z = linear(x, g.lin_src.weight)
        slope, rest = self._epilogue()
        out = mlgnn_gat.gat_aggregate(z, g.att_src, g.att_dst, g.bias, graph, g.heads, g.negative_slope, slope)
        for m in rest:
            out = m(out)
        return out if row_scale is None else out * row_scale.reshape(-1, 1)


class GraphConv(nn.Module):
    """Static graph convolution dispatcher (torch_vertex.py:338-363)."""

    def __init__(self, in_channels, out_channels, conv='edge', act='relu', norm=None, bias=True, heads=8,
                 mlp_norm=None, drop=0.0):
        super().__init__()
        kind = conv.lower()
        if kind == 'sage':
            self.gconv = RSAGEConv(in_channels, out_channels, act, norm, mlp_norm, bias, False, drop)
        elif kind == 'rsage':
            self.gconv = RSAGEConv(in_channels, out_channels, act, norm, mlp_norm, bias, True, drop)
        elif kind == 'gat':
            self.gconv = GATConv(in_channels, out_channels // heads, act, norm, bias, heads)
        elif kind in ('edge', 'mr', 'gcn', 'gin'):
            raise NotImplementedError('conv {} needs PyG layers outside the accelerated path'.format(conv))
        else:
            raise NotImplementedError('conv {} is not implemented'.format(conv))

    def forward(self, x, edge_index, edge_attr=None, row_scale=None, shared=None):
        return self.gconv(x, edge_index, edge_attr=edge_attr, row_scale=row_scale, shared=shared)
