"""DeeperGCN on the HIP CSR kernels (interface of the reference's ``models/deepergcn.py``:
class ``DeeperGCN`` :17, ``forward`` :185-323, ``print_params`` :325).

Same constructor ``(args)``, same ``forward(batch) -> softmax probabilities [B, num_tasks]``, same
``state_dict`` keys.  Differences in HOW: the graph is sorted to CSR once per batch and shared by
all layers; a scalar raw edge attribute is carried as a rank-one term through both Linear edge
encoders (no ``[E, d]`` embedding, no per-layer edge GEMM); the per-graph Python loops with
device->host syncs of the pathway-global-node branch (:221,:290) are index arithmetic on device.

``pathway_readout='MSA'`` (:126-128, :296-305): ``BatchNorm1d(pathway_num)`` over the stacked pathway rows, one
``nn.TransformerEncoderLayer(hidden_channels, 8, batch_first=True)`` and the graph pooling over its tokens.  The layer
is :class:`MSAReadout`, a subclass of the stock module (same parameters, ``state_dict`` keys and initial values) whose
forward runs ``softmax(Q K^T / sqrt(D)) V`` as one HIP launch per direction (:func:`mlgnn.mha_attention`, csrc/mha.hip)
on the in-projection's output as it lies in memory, the Linears through :func:`mlgnn.dense.linear` (residual adds in
their epilogues) and the LayerNorms through :func:`mlgnn.norm.layer_norm_act`.  ``MLGNN_MSA_FUSED=0`` runs the attention
as torch ops on the device instead (A/B runs).
"""
import logging
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from mlgnn import CSRGraph, LowRankEdge
from mlgnn import TableEdge, share_edge_gradient
from mlgnn.dense import linear
from mlgnn.mha import mha_attention, mha_supported
from mlgnn.norm import layer_norm_act, layer_norm_act_fork
from mlgnn.pool import global_pool
from mlgnn.pool_flatten import module_pool_flatten
from .gcn_lib.sparse.torch_vertex import GENConv
from .gcn_lib.sparse.torch_nn import norm_layer

MSA_FUSED = os.environ.get("MLGNN_MSA_FUSED", "1") == "1"      # (0: the attention of MSAReadout as torch ops, for A/B runs)


def torch_attention(qkv, batch, heads, keep=None, keep_scale=1.0):
    """What :func:`mlgnn.mha_attention` computes, in torch ops on the device of ``qkv`` (shapes the kernels refuse,
    ``MLGNN_MSA_FUSED=0``)."""
    B, H = int(batch), int(heads)
    P, D = qkv.shape[0] // B, qkv.shape[1] // (3 * H)
    q, k, v = qkv.reshape(B, P, 3, H, D).permute(2, 0, 3, 1, 4)              # [B, H, P, D] each
    a = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(D), dim=-1)
    if keep is not None:
        a = a * (keep.to(a.dtype) * keep_scale)
    return torch.matmul(a, v).transpose(1, 2).reshape(B * P, H * D)


class MSAReadout(nn.TransformerEncoderLayer):
    """``nn.TransformerEncoderLayer`` (post-norm, ReLU, batch first) with the forward on the HIP path; parameters,
    ``state_dict`` keys and initial values are the stock module's by construction.  The dropout masks are drawn by
    torch's generator (the attention's as a byte mask the kernel multiplies in)."""

    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0.1, batch_first=True):
        if not batch_first:
            raise NotImplementedError("MSAReadout is batch first, as the reference builds the layer")
        super().__init__(d_model=d_model, nhead=nhead, dim_feedforward=dim_feedforward, dropout=dropout,
                         batch_first=True)

    def _attention(self, qkv, B):
        at = self.self_attn
        P = qkv.shape[0] // B
        keep, scale = None, 1.0
        if self.training and at.dropout > 0:
            p = float(at.dropout)
            keep = torch.empty((B, at.num_heads, P, P), dtype=torch.uint8, device=qkv.device)
            keep, scale = (keep.zero_(), 0.0) if p >= 1.0 else (keep.bernoulli_(1.0 - p), 1.0 / (1.0 - p))
        if MSA_FUSED and mha_supported(qkv, B, at.num_heads):
            return mha_attention(qkv, B, at.num_heads, keep, scale)
        return torch_attention(qkv, B, at.num_heads, keep, scale)

    def forward(self, src, src_mask=None, src_key_padding_mask=None, is_causal=False):
        if src_mask is not None or src_key_padding_mask is not None or is_causal:
            raise NotImplementedError("MSAReadout attends over all tokens (no masks), as the reference calls the layer")
        B, P, d = src.shape
        at = self.self_attn
        x = src.reshape(B * P, d)
        qkv = linear(x, at.in_proj_weight, at.in_proj_bias)
        o = self._attention(qkv, B)
        if self.training and self.dropout1.p > 0:
            y = x + self.dropout1(linear(o, at.out_proj.weight, at.out_proj.bias))
        else:
            y = linear(o, at.out_proj.weight, at.out_proj.bias, residual=x)
        y = layer_norm_act(y, self.norm1.weight, self.norm1.bias, self.norm1.eps)
        f = self.dropout(F.relu(linear(y, self.linear1.weight, self.linear1.bias)))
        if self.training and self.dropout2.p > 0:
            f = y + self.dropout2(linear(f, self.linear2.weight, self.linear2.bias))
        else:
            f = linear(f, self.linear2.weight, self.linear2.bias, residual=y)
        return layer_norm_act(f, self.norm2.weight, self.norm2.bias, self.norm2.eps).reshape(B, P, d)


class DeeperGCN(torch.nn.Module):
    def __init__(self, args):
        super().__init__()
        self.num_layers = args.num_layers
        self.dropout = args.dropout
        self.block = args.block
        self.mul_attr = args.mul_attr
        hidden_channels = args.hidden_channels
        self.hidden_channels = hidden_channels
        self.learn_t = args.learn_t
        self.learn_p = args.learn_p
        self.msg_norm = args.msg_norm
        if self.block not in ('res+', 'res', 'plain'):
            if self.block == 'dense':
                raise NotImplementedError('To be implemented')
            raise Exception('Unknown block Type')
        if args.conv != 'gen':
            raise Exception('Unknown Conv Type')
        if args.gnn_encoder != 'linear':
            raise NotImplementedError("gnn_encoder=%r is outside the accelerated path" % (args.gnn_encoder,))
        if args.pathway_global_node and args.pathway_readout not in (None, 'maxpool', 'MSA'):
            raise NotImplementedError("pathway_readout=%r is outside the accelerated path" % (args.pathway_readout,))

        self.pca_only = args.pca_only
        self.gnn_encoder = args.gnn_encoder
        self.no_inter_drop = args.no_inter_drop
        self.no_inter_norm = args.no_inter_norm
        self.feature_drop_flag = args.feature_drop

        self.gcns = torch.nn.ModuleList()
        self.norms = torch.nn.ModuleList()
        for _ in range(self.num_layers):
            self.gcns.append(GENConv(hidden_channels, hidden_channels, aggr=args.gcn_aggr, t=args.t,
                                     learn_t=self.learn_t, p=args.p, learn_p=self.learn_p,
                                     gnn_encoder=self.gnn_encoder, msg_norm=self.msg_norm,
                                     learn_msg_scale=args.learn_msg_scale, encode_edge=args.conv_encode_edge,
                                     edge_feat_dim=hidden_channels, norm=args.norm, mlp_layers=args.mlp_layers,
                                     pca_only=self.pca_only))
            self.norms.append(norm_layer(args.norm, hidden_channels))

        self.node_embedding = args.node_embedding
        if self.node_embedding:
            self.node_embedding_encoder = torch.nn.Embedding(args.node_num, args.node_embedding_dim)
        input_dim = 3 + (args.node_embedding_dim if self.node_embedding else 0) + (2 if self.mul_attr else 0)
        self.node_features_encoder = torch.nn.Linear(input_dim, hidden_channels)
        self.edge_encoder = torch.nn.Linear(7 if args.use_column is None else 1, hidden_channels)

        self.global_edge = args.global_edge
        if args.global_edge == "onehot":
            self.edge_encoder = torch.nn.Embedding(args.pathway_edge_num, hidden_channels)

        self.use_edge_attr = args.use_edge_attr
        self.pathway_global_node = args.pathway_global_node
        if self.pathway_global_node:
            self.pathway_num = args.pathway_num
            self.pathway_features_encoder = torch.nn.Linear(6, hidden_channels)

        self.num_layer_head = args.num_layer_head
        self.pathway_readout = args.pathway_readout
        self.pre_concat_age = args.pre_concat_age
        self.feature_drop = nn.Dropout(0.25)
        if self.pathway_global_node and self.pathway_readout == 'maxpool':
            readout_in = (self.pathway_num // 4) * hidden_channels + (1 if args.pre_concat_age else 0)
            mods = [nn.Linear(readout_in, hidden_channels), nn.ReLU()]
            if not args.pre_readout_drop:
                mods.append(nn.Dropout(0.5))
            self.readout_func = nn.Sequential(*mods)
        elif self.pathway_global_node and self.pathway_readout == 'MSA':
            self.pred_norm = nn.BatchNorm1d(self.pathway_num)
            self.readout_func = MSAReadout(hidden_channels, 8, batch_first=True)

        if args.graph_pooling not in ("sum", "mean", "max"):
            raise Exception('Unknown Pool Type')
        self.graph_pooling = args.graph_pooling

        self.graph_pred_linear = torch.nn.Sequential()
        self.use_age = args.use_age
        head_embedding = (hidden_channels + 1) if args.use_age and not args.pre_concat_age else hidden_channels
        for i in range(args.num_layer_head - 1):
            self.graph_pred_linear.add_module(str(2 * i), torch.nn.Linear(head_embedding, head_embedding))
            self.graph_pred_linear.add_module(str(2 * i + 1), torch.nn.ReLU())
            if args.head_dropout:
                self.graph_pred_linear.add_module("drop{}".format(str(i)), torch.nn.Dropout(self.dropout))
        self.graph_pred_linear.add_module(str(2 * args.num_layer_head), torch.nn.Linear(head_embedding, args.num_tasks))

        if args.all_init:
            self.init_weight()
        elif args.head_init:
            for m in self.graph_pred_linear.modules():
                if isinstance(m, nn.Linear):
                    nn.init.xavier_uniform_(m.weight.data)
                    torch.nn.init.constant_(m.bias.data, 0.0)

    # ------------------------------------------------------------------ helpers
    def _edge_term(self, edge_attr):
        """Model-level edge embedding (deepergcn.py:212-215), kept factored (<= 8 raw attribute columns:
        both the 7-column default and the single ``use_column`` one) so no [E, H] tensor is built."""
        if not self.use_edge_attr:
            return None
        if self.global_edge == "onehot":
            idx = edge_attr.to(torch.long)
            enc = self.edge_encoder
            if (idx.dim() == 2 and idx.shape[1] == 1 and enc.padding_idx is None and enc.max_norm is None
                    and enc.weight.is_cuda and enc.weight.dtype == torch.float32):
                # [E, 1, H] flattened = table[idx]: kept as (table, row per edge); the kernels read the table rows
                return TableEdge(enc.weight, idx[:, 0], source=edge_attr)
            emb = enc(idx).flatten(1)
        elif edge_attr.dim() == 2 and 1 <= edge_attr.shape[1] <= LowRankEdge.MAX_RANK:
            return LowRankEdge(edge_attr, self.edge_encoder.weight, self.edge_encoder.bias)
        else:
            emb = self.edge_encoder(edge_attr).flatten(1)
        # one dense embedding read by every layer: without per-layer edge encoders the layers' [E, H] edge gradients
        # meet in one buffer inside the backward kernels instead of in L-1 separate additions
        shared = self.num_layers > 1 and not any(getattr(g, "encode_edge", False) for g in self.gcns)
        return share_edge_gradient(emb) if shared else emb

    def _pathway_rows(self, node_size):
        """Row indices of the last ``pathway_num`` nodes of every graph, [B * pathway_num]."""
        ends = torch.cumsum(node_size.to(torch.long), dim=0)
        offs = torch.arange(-self.pathway_num, 0, device=ends.device)
        return (ends[:, None] + offs[None, :]).reshape(-1)

    def _drop(self, h):
        return F.dropout(h, p=self.dropout, training=self.training)

    def _norm(self, layer, h, relu=False, drop=False):
        """``norms[layer](h)`` (+ ReLU) (+ the dropout behind it): one fused HIP pass for LayerNorm, the modules
        otherwise."""
        m = self.norms[layer]
        p = self.dropout if (drop and self.training) else 0.0
        if isinstance(m, nn.LayerNorm):
            return layer_norm_act(h, m.weight, m.bias, m.eps, relu, dropout_p=p)
        h = m(h)
        h = F.relu(h) if relu else h
        return self._drop(h) if drop else h

    def _res_plus_unfused(self, h, graph, edge_emb):
        """res+ stack with the norm / ReLU / dropout passes of their own (dropout active, non-LayerNorm norms)."""
        L = self.num_layers
        h = self.gcns[0](h, graph, edge_emb)
        for layer in range(1, L):
            m = self.norms[layer - 1]
            drop = not self.no_inter_drop
            if not self.no_inter_norm and isinstance(m, nn.LayerNorm) and h.dim() == 2:
                # the residual add runs in the conv's last GEMM epilogue and its gradient inside the
                # LayerNorm backward kernel (same values, two elementwise passes fewer); the dropout behind
                # norm + ReLU is applied by the same kernels
                h2, identity = layer_norm_act_fork(h, m.weight, m.bias, m.eps, relu=True,
                                                   dropout_p=self.dropout if (drop and self.training) else 0.0)
            else:
                h2 = F.relu(h) if self.no_inter_norm else self._norm(layer - 1, h, relu=True)
                identity = h
                if drop:
                    h2 = self._drop(h2)
            h = self.gcns[layer](h2, graph, edge_emb, residual=identity)
        h = self._norm(L - 1, h, drop=not self.no_inter_drop)
        return h

    # ------------------------------------------------------------------ forward
    def forward(self, input_batch):
        x = input_batch.x
        if self.pca_only:
            raise NotImplementedError("pca_only is outside the accelerated path")
        graph = getattr(input_batch, "csr", None)
        if graph is None:
            # the SAME edge_index tensor again (a training loop over one graph, a reused batch): the CSR built the first
            # time (identity + version match, no device work); a fresh tensor builds as before
            graph = CSRGraph.from_cache(input_batch.edge_index, x.shape[0])
        batch = input_batch.batch
        age = input_batch.age

        if self.node_embedding:
            emb = self.node_embedding_encoder(x[:, -1].to(torch.long))
            h = linear(torch.cat([x[:, :-1], emb], dim=-1), self.node_features_encoder.weight,
                       self.node_features_encoder.bias)
        else:
            h = linear(x, self.node_features_encoder.weight, self.node_features_encoder.bias)
        edge_emb = self._edge_term(input_batch.edge_attr)

        rows = None
        if self.pathway_global_node:
            pemb = self.pathway_features_encoder(input_batch.pathway_node_attr)
            rows = self._pathway_rows(input_batch.node_size)
            h = h.index_copy(0, rows, pemb.reshape(-1, pemb.shape[-1]))

        L = self.num_layers
        if self.block == 'res+':
            drop_active = self.training and self.dropout > 0 and not self.no_inter_drop
            if (not self.no_inter_norm and not drop_active and h.dim() == 2
                    and all(isinstance(m, nn.LayerNorm) and m.elementwise_affine for m in self.norms)):
                # every conv also emits the norm (+ ReLU) of its result -- the next block's input, or the final norm --
                # from its last GEMM's epilogue (mlgnn.dense._FusedMLP2 `post`): no LayerNorm pass of its own; the
                # residual add runs in the same epilogue and its gradient inside that LayerNorm's backward
                h, y = self.gcns[0](h, graph, edge_emb, post_norm=(self.norms[0], L > 1))
                for layer in range(1, L):
                    h, y = self.gcns[layer](y, graph, edge_emb, residual=h, post_norm=(self.norms[layer], layer < L - 1))
                h = y
            else:
                h = self._res_plus_unfused(h, graph, edge_emb)
        elif self.block == 'res':
            h = self._drop(self._norm(0, self.gcns[0](h, graph, edge_emb), relu=True))
            for layer in range(1, L):
                h = self._norm(layer, self.gcns[layer](h, graph, edge_emb), relu=True) + h
                h = self._drop(h)
        else:  # plain
            h = self._drop(self._norm(0, self.gcns[0](h, graph, edge_emb), relu=True))
            for layer in range(1, L):
                h1 = self.gcns[layer](h, graph, edge_emb)
                relu = layer != L - 1
                h = (F.relu(h1) if relu else h1) if self.no_inter_norm else self._norm(layer, h1, relu=relu)
                if not self.no_inter_drop:
                    h = self._drop(h)

        n_graphs = int(age.shape[0]) if age is not None else None
        if self.pathway_global_node:
            prow = h.index_select(0, rows)
            if self.pathway_readout is None:
                h_graph = global_pool(prow, batch.index_select(0, rows), self.graph_pooling, n_graphs)
            elif self.pathway_readout == 'MSA':
                prow = self.readout_func(self.pred_norm(prow.reshape(-1, self.pathway_num, h.shape[-1])))
                h_graph = global_pool(prow.reshape(-1, h.shape[-1]), batch.index_select(0, rows), self.graph_pooling,
                                      n_graphs)
            else:  # maxpool
                prow = prow.reshape(-1, self.pathway_num, h.shape[-1])
                if self.feature_drop_flag:
                    prow = self.feature_drop(prow)
                # (max_pool1d(prow^T, 4), flatten, cat with age: prow [B, P, d] is the channel-last image
                # [B, C = d, H = P, W = 1] under the window (4, 1); feature_drop acts before the pool, so no dropout here)
                h_graph = module_pool_flatten((4, 1), None, prow.transpose(1, 2).unsqueeze(-1),
                                              age if self.pre_concat_age else None)
                h_graph = self.readout_func(h_graph)
        else:
            h_graph = global_pool(h, batch, self.graph_pooling, n_graphs)

        if self.use_age and not self.pre_concat_age:
            h_graph = torch.cat([h_graph, age[:, None]], dim=-1)
        return F.softmax(self.graph_pred_linear(h_graph), dim=-1)

    def print_params(self, epoch=None, final=False):
        for flag, attr, tag in ((self.learn_t, 't', 't'), (self.learn_p, 'p', 'p')):
            if flag:
                vals = [getattr(g, attr).item() for g in self.gcns]
                print('Final {} {}'.format(tag, vals)) if final else logging.info('Epoch {}, {} {}'.format(epoch, tag, vals))
        if self.msg_norm:
            ss = [g.msg_norm.msg_scale.item() for g in self.gcns]
            print('Final s {}'.format(ss)) if final else logging.info('Epoch {}, s {}'.format(epoch, ss))

    def init_weight(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.xavier_uniform_(m.weight.data)
                torch.nn.init.constant_(m.bias.data, 0.0)
